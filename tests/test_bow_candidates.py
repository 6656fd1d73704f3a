"""The list form of the relocalisation search (orbx_bowdb_search_candidates_device[_compact], k_bow2_cand in orb-slam2_amd/csrc/orbx_bow.hip):
SearchByBoW(pKF, F) for the (frame, candidate) pairs that device-resident candidate lists name, as the loop of Tracking::Relocalization
runs it (src/Tracking.cc:1661-1682) -- one launch, the lists never read by the host.

Every output is filled with a sentinel before a launch (-7 rows and lists, -9 counts), so that "left untouched" and "-1" are both visible.
A searched slot is compared with the CPU oracle's SearchByBoW for its (keyframe, frame) AND, byte for byte over the whole row or list
(the untouched tail included), with what the all-keyframes search writes for that keyframe on the same frames."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tools import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
B, CAP, NKF, STRIDE = 4, 384, 11, 5
COUNTS = [384, 0, 257, 300]            # a full frame, a featureless one, one past a 256-thread stride, an ordinary one
KF_BASE = [0, 3, 2, 0, 3, 3, 2, 0, 2, 3, 0]     # the frame a keyframe is a shuffled, bit-flipped view of
KF_NOFLAGS = 3                         # this keyframe has no map point at all
# ids are indices: the last keyframe, a duplicate, unordered ids, a negative id | a searched slot on the featureless frame | an empty list |
# a count above the stride, an id equal to the number of keyframes, a huge id
LISTS = [[10, 0, 10, 3, -1], [2, 0, 0, 0, 0], [0, 0, 0, 0, 0], [1, 11, 2147483647, 4, 5]]
NCAND = [5, 1, 0, 9]
# through the id map: 20 ids, holes, one entry beyond the keyframes; lists with an id >= n_ids, a hole, a negative id, a negative count
N_IDS = 20
KF_OF_ID = {17: 10, 4: 0, 9: 3, 12: 1, 0: 4, 19: 5, 6: 2, 3: 11, 8: 7}
MAP_LISTS = [[17, 4, 20, 9, 5], [6, 0, 0, 0, 0], [17, 4, 9, 12, 0], [12, 3, -5, 0, 19]]
MAP_NCAND = [5, 1, -3, 5]


def slot_keyframes(lists, ncand, kf_of_id=None, n_ids=0):
    """the keyframe index every slot searches, or -1 (include/orbx.h)"""
    out = np.full((len(lists), STRIDE), -1, np.int64)
    for b, ids in enumerate(lists):
        for j in range(min(max(ncand[b], 0), STRIDE)):
            kf = ids[j] if kf_of_id is None else (kf_of_id.get(ids[j], -1) if 0 <= ids[j] < n_ids else -1)
            out[b, j] = kf if 0 <= kf < NKF else -1
    return out


def synthetic(oracle):
    """frames and keyframes of bit-flipped copies of 120 prototype descriptors, so that matches exist; FeatureVectors by the oracle"""
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
    return dict(par=par, leaf=leaf, nd=nd, w=w, desc=desc, angle=angle, frames=frames, kfs=kfs)


def oracle_rows(oracle, data, kf_of_slot):
    """{(b, kf): (row, count)} for the searched slots"""
    return {(b, int(kf)): oracle.search_by_bow_kf_f(data["kfs"][int(kf)], data["frames"][b], 0.75, True)
            for b in range(B) for kf in kf_of_slot[b] if kf >= 0}


@pytest.fixture(scope="module")
def data(oracle):
    d = synthetic(oracle)
    d["expect"] = oracle_rows(oracle, d, slot_keyframes(LISTS, NCAND))
    d["expect"].update(oracle_rows(oracle, d, slot_keyframes(MAP_LISTS, MAP_NCAND, KF_OF_ID, N_IDS)))
    return d


def test_synthetic_scene_is_not_empty(oracle, data):
    """checks the fixture, not the feature (it needs neither the new entry points nor a GPU): the conditions that keep the list tests from
    being empty hold for the oracle alone: the searched slots of the frames that have
    features average at least 20 matches, a list capacity of 8 cuts at least one list, and the slots cover what the lists are there for"""
    kf = slot_keyframes(LISTS, NCAND)
    assert kf.tolist() == [[10, 0, 10, 3, -1], [2, -1, -1, -1, -1], [-1] * 5, [1, -1, -1, 4, 5]]
    assert slot_keyframes(MAP_LISTS, MAP_NCAND, KF_OF_ID, N_IDS).tolist() == [[10, 0, -1, 3, -1], [2, -1, -1, -1, -1], [-1] * 5, [1, -1, -1, 4, 5]]
    cnt = [data["expect"][(b, int(k))][1] for b in range(B) for k in kf[b] if k >= 0 and COUNTS[b] > 0]
    assert len(cnt) == 7 and np.mean(cnt) >= 20, cnt
    assert max(cnt) > 8
    assert data["expect"][(1, 2)][1] == 0 and data["expect"][(0, KF_NOFLAGS)][1] == 0


def test_symbols_declared_exported_and_mirrored(pkg):
    import __graft_entry__ as ge
    ge.build()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "orbx.h")).read(), flags=re.S)
    raw = C.CDLL(pkg.lib_path())
    for name, nargs in (("orbx_bowdb_search_candidates_device", 13), ("orbx_bowdb_search_candidates_device_compact", 14)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert m, f"{name} is not declared in include/orbx.h"
        assert len(m.group(1).split(",")) == nargs
        assert hasattr(raw, name), f"{name} is not exported"
        at = getattr(pkg.lib(), name).argtypes
        assert at is not None and len(at) == nargs, name
        assert at[8] is C.c_float and at[4] is C.c_int and at[7] is C.c_int
    assert callable(pkg.BowFrames.search_candidates) and callable(pkg.BowFrames.search_candidates_compact)


# ------------------------------------------------------------------------------------------ GPU

class Scene:
    """the synthetic frames resident in a BowFrames, the keyframes in a BowDatabase, and the all-keyframes search of the three output forms"""

    def __init__(self, pkg, data):
        import torch
        self.torch = torch
        kps = np.zeros((B, CAP, 7), np.float32)
        kps[:, :, 3] = data["angle"]                                  # cv::KeyPoint.angle, the only field the transform reads
        self.d_kps = torch.from_numpy(kps).cuda(); self.d_desc = torch.from_numpy(data["desc"]).cuda()
        self.d_n = torch.tensor(COUNTS, dtype=torch.int32, device="cuda")
        self.stream = torch.cuda.Stream(); self.st = self.stream.cuda_stream
        self.voc = pkg.ORBVocabulary(10, 4, data["par"], data["leaf"], data["nd"], data["w"])
        self.fr = pkg.BowFrames(B, CAP)
        torch.cuda.synchronize()
        self.fr.transform(self.voc, self.d_kps.data_ptr(), self.d_desc.data_ptr(), self.d_n.data_ptr(), B, 2, self.st)
        self.stream.synchronize()
        self.db = pkg.BowDatabase(data["kfs"])
        self.all = {}
        for form, width in (("dense", CAP), ("compact", 2 * CAP), ("compact8", 16)):
            m = torch.full((B, NKF, width), -7, dtype=torch.int32, device="cuda"); nm = torch.full((B, NKF), -9, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            if form == "dense":
                self.fr.search(self.db, B, m.data_ptr(), nm.data_ptr(), 0.75, True, self.st)
            else:
                self.fr.search_compact(self.db, B, m.data_ptr(), width // 2, nm.data_ptr(), 0.75, True, self.st)
            self.stream.synchronize()
            self.all[form] = (m.cpu().numpy(), nm.cpu().numpy())

    def run(self, form, lists, ncand, kf_of_id=None, n_ids=0):
        torch = self.torch
        width = {"dense": CAP, "compact": 2 * CAP, "compact8": 16}[form]
        d_cand = torch.tensor(lists, dtype=torch.int32, device="cuda"); d_nc = torch.tensor(ncand, dtype=torch.int32, device="cuda")
        d_map = None
        if kf_of_id is not None:
            d_map = torch.tensor([kf_of_id.get(i, -1) for i in range(n_ids)], dtype=torch.int32, device="cuda")
        m = torch.full((B, STRIDE, width), -7, dtype=torch.int32, device="cuda"); nm = torch.full((B, STRIDE), -9, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        kw = dict(nnratio=0.75, checkOri=True, kf_of_id=None if d_map is None else d_map.data_ptr(), n_ids=n_ids, stream=self.st)
        if form == "dense":
            self.fr.search_candidates(self.db, B, d_cand.data_ptr(), STRIDE, d_nc.data_ptr(), m.data_ptr(), nm.data_ptr(), **kw)
        else:
            self.fr.search_candidates_compact(self.db, B, d_cand.data_ptr(), STRIDE, d_nc.data_ptr(), m.data_ptr(), width // 2, nm.data_ptr(), **kw)
        self.stream.synchronize()
        return m.cpu().numpy(), nm.cpu().numpy()


@pytest.fixture(scope="module")
def scene(pkg, data):
    return Scene(pkg, data)


def check(scene, data, form, got, kf_of_slot):
    m, nm = got
    am, anm = scene.all[form]
    searched = cut = 0
    for b in range(B):
        n = COUNTS[b]
        for j in range(STRIDE):
            kf = int(kf_of_slot[b, j])
            if kf < 0:
                assert nm[b, j] == -1 and (m[b, j] == -7).all(), (form, b, j)
                continue
            exp, en = data["expect"][(b, kf)]
            assert nm[b, j] == en, (form, b, j, kf, int(nm[b, j]), en)
            if form == "dense":
                assert (m[b, j, :n] == exp).all() and (m[b, j, n:] == -7).all(), (form, b, j, kf)
            else:
                slots = np.nonzero(exp >= 0)[0]
                keep = min(en, m.shape[2] // 2)
                lst = m[b, j].reshape(-1, 2)
                assert (lst[:keep, 0] == slots[:keep]).all() and (lst[:keep, 1] == exp[slots[:keep]]).all() and (lst[keep:] == -7).all(), (form, b, j, kf)
                cut += en > keep
            assert nm[b, j] == anm[b, kf] and m[b, j].tobytes() == am[b, kf].tobytes(), (form, b, j, kf)      # the all-keyframes row, tail included
            searched += 1
    assert searched == int((kf_of_slot >= 0).sum()) >= 7
    if form == "compact8":
        assert cut >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["dense", "compact", "compact8"])
def test_hand_written_lists(pkg, data, scene, form):
    """ids that are indices: duplicates, unordered and negative ids, an id equal to and far above the number of keyframes, a count above the
    stride, an empty list, a searched slot on a featureless frame, a keyframe without map points"""
    check(scene, data, form, scene.run(form, LISTS, NCAND), slot_keyframes(LISTS, NCAND))


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["dense", "compact", "compact8"])
def test_id_map(pkg, data, scene, form):
    """the same keyframes through d_kf_of_id[20]: a permutation with holes, an entry beyond the keyframes, list ids >= n_ids and < 0, and a
    negative count (reads as 0) in front of a list that would otherwise be searched"""
    check(scene, data, form, scene.run(form, MAP_LISTS, MAP_NCAND, KF_OF_ID, N_IDS), slot_keyframes(MAP_LISTS, MAP_NCAND, KF_OF_ID, N_IDS))


@pytest.mark.gpu
def test_argument_refusals(pkg, data, scene):
    """every ORBX_E_INVALID case returns that code and launches nothing: the outputs keep their sentinels.  Two refusals are out of reach here:
    frames of another device are tried only where a second GPU exists, and the LDS-size refusal cannot be provoked through the ABI at all
    (orbx_bow_frames_create caps a frame at 8192 features = 82 KB of LDS, below the 120 KB limit bow_launch and this launch share)."""
    import torch
    L = pkg.lib()
    d_cand = torch.tensor(LISTS, dtype=torch.int32, device="cuda"); d_nc = torch.tensor(NCAND, dtype=torch.int32, device="cuda")
    d_map = torch.zeros(N_IDS, dtype=torch.int32, device="cuda")
    m = torch.full((B, STRIDE, 2 * CAP), -7, dtype=torch.int32, device="cuda"); nm = torch.full((B, STRIDE), -9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    db, fr, st = scene.db._h, scene.fr._h, scene.st
    cand, nc, out, cnt, idmap = d_cand.data_ptr(), d_nc.data_ptr(), m.data_ptr(), nm.data_ptr(), d_map.data_ptr()
    many = pkg.BowFrames(65536, 8)                      # untransformed: only its max_batch is looked at before the refusal
    # (db, frames, batch, d_cand, cand_stride, d_ncand, d_kf_of_id, n_ids, d_out, cap_pairs, d_nmatches)
    good = (db, fr, B, cand, STRIDE, nc, None, 0, out, CAP, cnt)
    bad = {"db": (0, None), "frames": (1, None), "d_cand": (3, None), "d_ncand": (5, None), "output": (8, None), "d_nmatches": (10, None),
           "batch 0": (2, 0), "batch -1": (2, -1), "batch above the frames'": (2, B + 1), "cand_stride 0": (4, 0), "cand_stride -1": (4, -1),
           "map without n_ids": [(6, idmap), (7, 0)], "map with negative n_ids": [(6, idmap), (7, -4)],
           "grid x": (4, 1 << 24), "grid y": [(1, many._h), (2, 65536)]}
    for name, edits in bad.items():
        a = list(good)
        for pos, val in (edits if isinstance(edits, list) else [edits]):
            a[pos] = val
        for compact in (0, 1):
            if compact:
                rc = L.orbx_bowdb_search_candidates_device_compact(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], 0.75, 1, a[8], a[9], a[10], st)
            else:
                rc = L.orbx_bowdb_search_candidates_device(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], 0.75, 1, a[8], a[10], st)
            assert rc == E_INVALID, (name, compact, rc)
    for cap_pairs in (0, -2):
        assert L.orbx_bowdb_search_candidates_device_compact(db, fr, B, cand, STRIDE, nc, None, 0, 0.75, 1, out, cap_pairs, cnt, st) == E_INVALID
    if L.orbx_device_count() > 1:                       # frames of another device
        other = pkg.BowFrames(B, CAP, device=1)
        assert L.orbx_bowdb_search_candidates_device(db, other._h, B, cand, STRIDE, nc, None, 0, 0.75, 1, out, cnt, st) == E_INVALID
    with pytest.raises(pkg.OrbxError) as ei:            # and through the mirror
        scene.fr.search_candidates(scene.db, B, cand, 0, nc, out, cnt, stream=st)
    assert ei.value.code == E_INVALID
    scene.stream.synchronize(); torch.cuda.synchronize()
    assert (m == -7).all().item() and (nm == -9).all().item()


@pytest.mark.gpu
def test_chain_on_one_stream(pkg, oracle):
    """extract -> transform -> orbx_kfdb_detect_relocalization_batch_device -> orbx_bowdb_search_candidates_device_compact on ONE stream with
    no host step between the last two (the scene of test_kfdb.py's resident-frames test): the candidates are the transcription model's, and
    every searched list is the oracle's SearchByBoW and the per-call resident search on the downloaded ids"""
    import torch
    import kfdb_model as km
    W, H, NB = 640, 480, 8
    base = [synth.image(300 + i, W, H) for i in range(3)]
    rng = np.random.default_rng(5)
    imgs = []
    for i in range(NB):
        im = np.roll(base[i % 3], (int(rng.integers(-6, 7)), int(rng.integers(-6, 7))), (0, 1)).astype(np.int16)
        imgs.append(np.clip(im + rng.integers(-6, 7, im.shape), 0, 255).astype(np.uint8))
    d_img = torch.from_numpy(np.stack(imgs)).cuda()
    ex = pkg.ORBextractor(1000, 1.2, 8, 20, 7, device=0, max_size=(W, H), max_batch=NB)
    cap = ex.max_keypoints(W, H)
    d_kps = torch.zeros((NB, cap, 7), device="cuda"); d_desc = torch.zeros((NB, cap, 32), dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(NB, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream(); st = stream.cuda_stream
    torch.cuda.synchronize()
    ex.extract_batch_device(d_img.data_ptr(), H * W, W, NB, W, H, d_kps.data_ptr(), d_desc.data_ptr(), cap, d_n.data_ptr(), st)
    stream.synchronize()
    n = d_n.cpu().numpy(); desc = d_desc.cpu().numpy(); kps = d_kps.cpu().numpy().view(np.uint8).reshape(NB, cap, 28)
    par, leaf, nd, w = synth.vocab_tree(41, 10, 4, stop_frac=0.02, data=np.concatenate([desc[i, :n[i]] for i in range(3)]))
    voc = pkg.ORBVocabulary(10, 4, par, leaf, nd, w); ovoc = oracle.Vocabulary(10, 4, par, leaf, nd, w)
    fr = pkg.BowFrames(NB, cap)
    fr.transform(voc, d_kps.data_ptr(), d_desc.data_ptr(), d_n.data_ptr(), NB, 4, st)
    vecs, sets = [], []
    for i in range(NB):
        t = ovoc.transform(desc[i, :n[i]], 4)
        vecs.append((t["bow_id"], t["bow_val"]))
        ang = np.frombuffer(kps[i, :n[i]].tobytes(), dtype=pkg.KP_DTYPE)["angle"].copy()
        sets.append(dict(desc=desc[i, :n[i]].copy(), node_id=t["fv_node_id"], node_off=t["fv_node_off"], feat=t["fv_feat"], angle=ang))
    nwords = voc.info()["words"]
    ref = km.RefDatabase(nwords); kfdb = pkg.KeyFrameDatabase(nwords)
    nkf = 5
    for i in range(nkf):                                           # frames 0..4 become keyframes 0..4, device to device: an id is the index
        assert kfdb.add(fr, i, stream=st) == ref.add(vecs[i]) == i
    for i in range(nkf):
        nb = [j for j in range(nkf) if j != i]
        kfdb.set_covisibility(i, nb); ref.set_covisibility(i, nb)
    kfs = [dict(sets[i], flag=(rng.random(n[i]) < 0.7).astype(np.uint8)) for i in range(nkf)]
    frames = [dict(s, flag=np.zeros(len(s["desc"]), np.uint8)) for s in sets]
    bowdb = pkg.BowDatabase(kfs)
    resident = [pkg.DeviceKeyFrame(k) for k in kfs]
    exp = [ref.DetectRelocalizationCandidates(v)[0] for v in vecs]
    stride = 8
    assert sum(min(len(e), stride) for e in exp) >= NB
    d_cand = torch.full((NB, stride), -1, dtype=torch.int32, device="cuda"); d_nc = torch.zeros(NB, dtype=torch.int32, device="cuda")
    d_pairs = torch.full((NB, stride, cap, 2), -7, dtype=torch.int32, device="cuda"); d_nm = torch.full((NB, stride), -9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    kfdb.detect_relocalization_batch_device(fr, NB, d_cand.data_ptr(), stride, d_nc.data_ptr(), st)
    fr.search_candidates_compact(bowdb, NB, d_cand.data_ptr(), stride, d_nc.data_ptr(), d_pairs.data_ptr(), cap, d_nm.data_ptr(), 0.75, True, stream=st)
    stream.synchronize()                                           # the only synchronisation, after both
    nc = d_nc.cpu().numpy(); cand = d_cand.cpu().numpy(); pairs = d_pairs.cpu().numpy(); nm = d_nm.cpu().numpy()
    assert [cand[i, :nc[i]].tolist() for i in range(NB)] == exp
    matcher = pkg.ORBmatcher(0.75, True)
    total = 0
    for i in range(NB):
        ids = [int(x) for x in cand[i, :min(nc[i], stride)]]
        assert (nm[i, len(ids):] == -1).all() and (pairs[i, len(ids):] == -7).all(), i
        if not ids:
            continue
        rows, cnt = matcher.SearchByBoWKeyFramesFrameResident([resident[k] for k in ids], [kfs[k]["flag"] for k in ids], frames[i])
        for j, k in enumerate(ids):
            orow, on = oracle.search_by_bow_kf_f(kfs[k], frames[i], 0.75, True)
            for name, row, count in (("oracle", orow, on), ("per call", rows[j], cnt[j])):
                slots = np.nonzero(row >= 0)[0]
                assert nm[i, j] == count == len(slots), (name, i, j, k)
                assert (pairs[i, j, :count, 0] == slots).all() and (pairs[i, j, :count, 1] == row[slots]).all(), (name, i, j, k)
            assert (pairs[i, j, on:] == -7).all(), (i, j, k)
            total += on
    assert total > 0
