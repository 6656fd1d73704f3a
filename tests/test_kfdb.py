"""Device-resident KeyFrameDatabase (orbx_kfdb_*, orb-slam2_amd/csrc/orbx_kfdb.hip): the place-recognition query of
Tracking::Relocalization (src/Tracking.cc:1650) and LoopClosing::DetectLoop (src/LoopClosing.cc:143-175).

CPU: the transcription of src/KeyFrameDatabase.cc (kfdb_model.RefDatabase) against the forward formulation the kernels use
(kfdb_model.ForwardDatabase) on a mixed sequence of adds, erases, covisibility updates and interleaved queries; L1 score known
answers; the no-GPU error; the adaptor's syntax check.  GPU: the library against RefDatabase, everything exact (candidate lists,
int32 words, float / double scores as bytes)."""
import os
import re
import struct
import subprocess
import threading

import numpy as np
import pytest

import kfdb_model as km
from tools import kfdb_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NWORDS = 100000
F32 = np.float32


# ------------------------------------------------------------------------------------------ the mixed sequence

def mixed_ops(seed=1):
    """adds, covisibility, interleaved relocalisation / loop queries and explicit scores; erases (some of them neighbours of live
    keyframes), re-adds under new ids, covisibility updates that name erased and not yet issued ids; clear and reuse"""
    sc = kfdb_scene.Scene(seed, nwords=NWORDS)
    n = len(sc.keyframes)
    rng = sc.rng
    ops = [("add", kf) for kf in sc.keyframes] + [("covis", i, sc.neighbours[i]) for i in range(n)]

    def mates(p):
        return [i for i in range(n) if sc.place_of[i] == p]

    def loop(p, second=None, scale=1.0):       # scale > 1: only keyframes of the place are connected, so minScore lands among the place's scores
        return ("loop", sc.query(p, second), mates(p)[:3] + [int(x) for x in rng.integers(0, n, 0 if scale > 1 else 2)], scale)

    for p in (0, 7, 13):
        ops.append(("reloc", sc.query(p)))
    ops += [loop(7, scale=1.1), ("reloc", sc.query(7)), ("reloc", sc.query(0)), loop(13, scale=0.5), ("reloc", sc.query(7, second=8)),
            ("score", sc.query(3), list(range(20, 40))), loop(0, second=1, scale=0.25), ("reloc", sc.query(13))]
    erased = [3, 11, 12, 40, 41, 58, 77, 100, 150, 199]
    ops += [("erase", i) for i in erased]
    ops += [("add", sc.keyframes[i]) for i in (3, 40, 150)]                   # ids n, n + 1, n + 2
    ops += [("covis", n, sc.neighbours[3]), ("covis", n + 1, [41, 42, 43, n, 12]), ("covis", 5, [11, n, 0, 1, 2, 4, 6, 7]),
            ("covis", 60, [58, 59, 61, 62, 63, 57, 56, n + 7])]
    for p in (0, 7, 5, 1, 7):
        ops.append(("reloc", sc.query(p)))
        ops.append(loop(p, scale=0.75 if p != 5 else 1.05))
    ops += [("score", sc.query(5), [0, 1, 2, n, n + 1, n + 2, 44, 45]), ("reloc", sc.query(5, second=7)), ("clear",)]
    ops += [("add", sc.keyframes[i]) for i in range(40)] + [("covis", i, sc.neighbours[i]) for i in range(40)]    # neighbours >= 40: unknown ids
    for p in (0, 4, 0, 2):
        ops.append(("reloc", sc.query(p)))
    ops.append(loop(4, scale=0.9))
    return ops


def run_ops(impl, ops, on_loop=None):
    """apply the sequence to a database with the model's interface; -> every observable result, scores as bytes"""
    live, trace = set(), []
    for op in ops:
        if op[0] == "add":
            i = impl.add(op[1]); live.add(i); trace.append(("add", i))
        elif op[0] == "erase":
            impl.erase(op[1]); live.discard(op[1])
        elif op[0] == "covis":
            impl.set_covisibility(op[1], op[2])
        elif op[0] == "clear":
            impl.clear(); live.clear()
        elif op[0] == "score":
            ids = [i for i in op[2] if i in live]
            trace.append(("score", ids, np.array(impl.score(op[1], ids), np.float64).tobytes()))
        elif op[0] == "reloc":
            c, w, s = impl.DetectRelocalizationCandidates(op[1])
            trace.append(("reloc", list(c), w.tobytes(), s.tobytes(), impl.reloc_scores().tobytes()))
        else:
            conn = [i for i in op[2] if i in live]
            sc = np.array(impl.score(op[1], conn), np.float64).astype(np.float32)      # src/LoopClosing.cc:143-162: minScore over the covisibles
            min_score = float(F32(sc.min() * F32(op[3])))
            if on_loop:
                on_loop(impl, op[1], op[2], min_score)
            c, w, s = impl.DetectLoopCandidates(op[1], op[2], min_score)
            trace.append(("loop", list(c), w.tobytes(), s.tobytes(), impl.reloc_scores().tobytes()))
    return trace


def scene_conditions(ref, connected_listed):
    """the scenes must exercise every branch of the two queries (asserted on the model before anything is compared with the GPU)"""
    st = ref.stats
    assert st["max_candidates"] >= 3, st
    assert st["gate_failed"] >= 1, st              # shares a word, fails the 0.8 gate
    assert st["groups_dropped"] >= 1, st           # 0.75 gate
    assert st["neighbour_best"] >= 1, st
    assert st["duplicates"] >= 1, st
    assert st["stale_nonzero"] >= 1, st
    assert st["below_min_score"] >= 1, st
    assert connected_listed[0] >= 1                # a connected keyframe that would have been returned


def _connected_probe(count):
    def probe(impl, q, connected, min_score):      # only the forward model is free of per-keyframe query state: ask it without the exclusion
        cands = impl.DetectLoopCandidates(q, [], min_score)[0]
        count[0] += len(set(cands) & set(connected))
    return probe


def reference_trace(ops):
    ref, fwd, listed = km.RefDatabase(NWORDS), km.ForwardDatabase(NWORDS), [0]
    ta = run_ops(ref, ops)
    tb = run_ops(fwd, ops, on_loop=_connected_probe(listed))
    return ref, ta, tb, listed


_cache = {}


def _mixed():
    if "mixed" not in _cache:
        ops = mixed_ops()
        _cache["mixed"] = (ops,) + reference_trace(ops)
    return _cache["mixed"]


# ------------------------------------------------------------------------------------------ CPU

def test_transcription_and_forward_form_agree():
    ops, ref, ta, tb, listed = _mixed()
    scene_conditions(ref, listed)
    assert len(ta) == len(tb)
    for k, (a, b) in enumerate(zip(ta, tb)):
        assert a == b, (k, a[0], a[1], b[1])
    assert sum(1 for t in ta if t[0] in ("reloc", "loop") and t[1]) >= 20


def test_l1_score_known_answers():
    sc = kfdb_scene.Scene(2, places=2, per_place=2, nwords=NWORDS)
    v = sc.keyframes[0]
    acc = 0.0
    for x in v[1]:
        x = float(x)
        acc += abs(x - x) - abs(x) - abs(x)
    same = km.l1_score(v, v)
    assert same == -acc / 2.0 and abs(same - 1.0) < 1e-12 and km.forward_score(v, v) == same
    a = (np.array([1, 5, 9], np.uint32), np.array([0.5, 0.25, 0.25]))
    b = (np.array([2, 6, 10], np.uint32), np.array([0.5, 0.25, 0.25]))
    assert km.l1_score(a, b) == 0.0 and km.forward_score(a, b) == 0.0
    # three words by hand: word 5 (|0.25 - 0.5| - 0.25 - 0.5 = -0.5) and word 9 (|0.25 - 0.125| - 0.25 - 0.125 = -0.25): 0.375
    c = (np.array([5, 9, 11], np.uint32), np.array([0.5, 0.125, 0.375]))
    assert km.l1_score(a, c) == 0.375 and km.forward_score(a, c) == 0.375
    # 12 decades: the sum depends on its order, and both models take the ascending word order
    ids = np.arange(0, 40, dtype=np.uint32)
    rng = np.random.default_rng(3)
    x = (ids, 10.0 ** rng.uniform(-12, 0, 40)); y = (ids, 10.0 ** rng.uniform(-12, 0, 40))
    fwd = km.l1_score(x, y)
    rev = 0.0
    for vi, wi in zip(x[1][::-1], y[1][::-1]):
        rev += abs(float(vi) - float(wi)) - abs(float(vi)) - abs(float(wi))
    assert fwd == km.forward_score(x, y) and fwd != -rev / 2.0


def test_no_gpu_raises(pkg):
    """no CPU fallback: without a device the handle cannot be created"""
    if pkg.lib().orbx_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(pkg.OrbxError) as ei:
        pkg.KeyFrameDatabase(NWORDS)
    assert ei.value.code == -4


ADAPTER_INC = ["-I", os.path.join(ROOT, "adapter"), "-I", os.path.join(ROOT, "tests", "cvstub_kfdb"), "-I", os.path.join(ROOT, "tests", "cvstub_rgbd"),
               "-I", os.path.join(ROOT, "tests", "cvstub"), "-I", os.path.join(ROOT, "include")]


def test_adapter_sources_compile():
    """adapter/KeyFrameDatabase.cc against the overlay (tests/cvstub_kfdb) in front of tests/cvstub, on the include path of the adaptor
    build line; the overlay stays a superset of the stub, so every other adaptor source compiles against it unchanged"""
    ad = os.path.join(ROOT, "adapter")
    for f in sorted(os.listdir(ad)):
        if f.endswith(".cc"):
            subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only"] + ADAPTER_INC + [os.path.join(ad, f)])


def test_adapter_build_line_has_one_keyframe_layout():
    """every translation unit of the adaptor build line (__graft_entry__.build: adapter/*.cc + tests/adapter_driver.cc, overlay in front) that
    sees a definition of ORB_SLAM2::KeyFrame sees the overlay's.  tests/cvstub/ORBmatcher.h names "KeyFrame.h" in quotes, which finds the
    stub's header beside it; without the overlay's ORBmatcher.h shim the matcher sources got the stub's class and the others the overlay's,
    two layouts in one program (examples/adapter_bench then read vectors at the wrong offsets)."""
    ad = os.path.join(ROOT, "adapter")
    srcs = [os.path.join(ad, f) for f in sorted(os.listdir(ad)) if f.endswith(".cc")] + \
        [os.path.join(ROOT, "tests", "adapter_driver.cc"), os.path.join(ROOT, "tests", "adapter_kfdb_driver.cc")]
    defining = 0
    for src in srcs:
        text = subprocess.run(["g++", "-std=c++11", "-E", "-DORBX_ADAPTER_CAPTURE"] + ADAPTER_INC + [src], capture_output=True, text=True, check=True).stdout
        if re.search(r"\bclass\s+KeyFrame\s*(:[^{;]*)?\{", text):       # a definition, however it is laid out (a forward declaration has no brace)
            defining += 1
            assert "mvpOrderedConnectedKeyFrames;" in text and "long unsigned int mnId;" in text, src
    assert defining >= 6


# ------------------------------------------------------------------------------------------ GPU

class GpuImpl:
    """the library behind the model's interface; with `frames`, every second add / query / score goes through an orbx_bow_frames slot
    (add_from_frames and the _frame query forms)"""

    def __init__(self, pkg, nwords, frames=None):
        self.db = pkg.KeyFrameDatabase(nwords)
        self.fr, self.k = frames, 0

    def _slot(self, bow):
        self.k += 1
        if self.fr is None or self.k % 2:
            return None
        self.fr.set_bow(self.k % self.fr.batch, bow)
        return self.k % self.fr.batch

    def add(self, bow):
        s = self._slot(bow)
        return self.db.add(bow) if s is None else self.db.add(self.fr, s)

    def erase(self, i): self.db.erase(i)
    def clear(self): self.db.clear()
    def set_covisibility(self, i, nb): self.db.set_covisibility(i, nb)
    def reloc_scores(self): return self.db.reloc_scores()

    def score(self, q, ids):
        s = self._slot(q)
        return self.db.score(q, ids) if s is None else self.db.score(self.fr, ids, index=s)

    def DetectRelocalizationCandidates(self, q):
        s = self._slot(q)
        return self.db.DetectRelocalizationCandidates(q, stages=True) if s is None else self.db.DetectRelocalizationCandidates(self.fr, index=s, stages=True)

    def DetectLoopCandidates(self, q, connected, min_score):
        s = self._slot(q)
        if s is None:
            return self.db.DetectLoopCandidates(q, connected, min_score, stages=True)
        return self.db.DetectLoopCandidates(self.fr, connected, min_score, index=s, stages=True)


def _same(got, exp):
    assert len(got) == len(exp)
    for k, (g, e) in enumerate(zip(got, exp)):
        assert g == e, (k, e[0], g[1], e[1])


@pytest.mark.gpu
def test_gpu_percall_parity(pkg):
    ops, ref, ta, tb, listed = _mixed()
    scene_conditions(ref, listed)
    _same(run_ops(GpuImpl(pkg, NWORDS, pkg.BowFrames(3, 2048)), ops), ta)
    _same(run_ops(GpuImpl(pkg, NWORDS), ops), ta)                  # host forms only


def _scene_db(impl, sc):
    for kf in sc.keyframes:
        impl.add(kf)
    for i, nb in enumerate(sc.neighbours):
        impl.set_covisibility(i, nb)


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 7, 32])
def test_gpu_batched_parity(pkg, batch):
    """orbx_kfdb_detect_relocalization_batch_device == the per-call queries in frame order, persistent scores included.  The batched form
    exposes no per-query words / scores, so those stages are compared through the per-call forms only (test_gpu_percall_parity); here the
    persistent scores after the batch stand for them: they are the scores of every keyframe's last scoring query."""
    import torch
    sc = kfdb_scene.Scene(20 + batch, nwords=NWORDS)
    places = [(3, None), (5, None), (3, None), (3, 5), (9, None), (5, None), (3, None)]
    queries = [sc.query(*places[i % len(places)]) for i in range(batch)]
    ref = km.RefDatabase(NWORDS); _scene_db(ref, sc)
    warm = [sc.query(3), sc.query(9)]                              # scores kept from before the batch
    percall = GpuImpl(pkg, NWORDS); _scene_db(percall, sc)
    batched = GpuImpl(pkg, NWORDS); _scene_db(batched, sc)
    for q in warm:
        e = ref.DetectRelocalizationCandidates(q)[0]
        assert percall.DetectRelocalizationCandidates(q)[0] == e and batched.DetectRelocalizationCandidates(q)[0] == e
    exp = [ref.DetectRelocalizationCandidates(q)[0] for q in queries]
    if batch >= 7:
        assert ref.stats["stale_nonzero"] >= 1 and ref.stats["neighbour_best"] >= 1 and max(len(e) for e in exp) >= 2, ref.stats
    assert [percall.DetectRelocalizationCandidates(q)[0] for q in queries] == exp
    fr = pkg.BowFrames(batch, 2048)
    for i, q in enumerate(queries):
        fr.set_bow(i, q)
    cap = 16
    d_cand = torch.full((batch, cap), -1, dtype=torch.int32, device="cuda"); d_n = torch.full((batch,), -1, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    batched.db.detect_relocalization_batch_device(fr, batch, d_cand.data_ptr(), cap, d_n.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    n = d_n.cpu().numpy(); cand = d_cand.cpu().numpy()
    assert [cand[i, :n[i]].tolist() for i in range(batch)] == exp
    want = ref.reloc_scores().tobytes()
    assert batched.reloc_scores().tobytes() == want and percall.reloc_scores().tobytes() == want


@pytest.mark.gpu
def test_gpu_batched_on_default_stream_then_percall(pkg):
    """frames that no transform has touched (filled by set_bow, stream NULL) queried with stream NULL: the batch runs on the default stream,
    and the per-call query issued at once on the same handle must wait for it (it reuses the workspace and reads the persistent scores the
    batch writes).  Repeated, so that an unordered overlap would show."""
    import torch
    sc = kfdb_scene.Scene(31, nwords=NWORDS)
    ref = km.RefDatabase(NWORDS); _scene_db(ref, sc)
    gpu = GpuImpl(pkg, NWORDS); _scene_db(gpu, sc)
    batch, cap = 32, 16
    fr = pkg.BowFrames(batch, 2048)
    d_cand = torch.full((batch, cap), -1, dtype=torch.int32, device="cuda"); d_n = torch.full((batch,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for rnd in range(6):
        queries = [sc.query((3 * i + rnd) % 5) for i in range(batch)]
        tail = sc.query(rnd % 5)
        for i, q in enumerate(queries):
            fr.set_bow(i, q)                       # stream=None
        exp = [ref.DetectRelocalizationCandidates(q)[0] for q in queries]
        exp_tail = ref.DetectRelocalizationCandidates(tail)
        gpu.db.detect_relocalization_batch_device(fr, batch, d_cand.data_ptr(), cap, d_n.data_ptr())     # stream=None
        got_tail = gpu.db.DetectRelocalizationCandidates(tail, stages=True)                               # at once, no synchronisation between
        assert got_tail[0] == exp_tail[0] and got_tail[1].tobytes() == exp_tail[1].tobytes() and got_tail[2].tobytes() == exp_tail[2].tobytes(), rnd
        torch.cuda.synchronize()
        n = d_n.cpu().numpy(); cand = d_cand.cpu().numpy()
        assert [cand[i, :n[i]].tolist() for i in range(batch)] == exp, rnd
        assert gpu.reloc_scores().tobytes() == ref.reloc_scores().tobytes(), rnd
    assert ref.stats["stale_nonzero"] >= 1


@pytest.mark.gpu
def test_gpu_device_chain(pkg, oracle):
    """extract -> orbx_bow_transform_batch_device -> add_from_frames / batched detect with no host copy in between, against the oracle's
    Vocabulary.transform on the downloaded descriptors + the transcription model"""
    import torch
    from tools import synth
    W, H, B = 640, 480, 8
    base = [synth.image(300 + i, W, H) for i in range(3)]
    rng = np.random.default_rng(5)
    imgs = []
    for i in range(B):                                             # views of three places: the same image under noise and a small shift
        im = np.roll(base[i % 3], (int(rng.integers(-6, 7)), int(rng.integers(-6, 7))), (0, 1)).astype(np.int16)
        imgs.append(np.clip(im + rng.integers(-6, 7, im.shape), 0, 255).astype(np.uint8))
    host = np.stack(imgs)
    d_img = torch.from_numpy(host).cuda()
    ex = pkg.ORBextractor(1000, 1.2, 8, 20, 7, device=0, max_size=(W, H), max_batch=B)
    cap = ex.max_keypoints(W, H)
    d_kps = torch.zeros((B, cap, 7), device="cuda"); d_desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(B, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream(); st = stream.cuda_stream
    torch.cuda.synchronize()
    ex.extract_batch_device(d_img.data_ptr(), H * W, W, B, W, H, d_kps.data_ptr(), d_desc.data_ptr(), cap, d_n.data_ptr(), st)
    stream.synchronize()
    n = d_n.cpu().numpy(); desc = d_desc.cpu().numpy()
    par, leaf, nd, w = synth.vocab_tree(41, 10, 4, stop_frac=0.02, data=np.concatenate([desc[i, :n[i]] for i in range(3)]))
    voc = pkg.ORBVocabulary(10, 4, par, leaf, nd, w); ovoc = oracle.Vocabulary(10, 4, par, leaf, nd, w)
    fr = pkg.BowFrames(B, cap)
    fr.transform(voc, d_kps.data_ptr(), d_desc.data_ptr(), d_n.data_ptr(), B, 4, st)
    vecs = []
    for i in range(B):
        t = ovoc.transform(desc[i, :n[i]], 4)
        vecs.append((t["bow_id"], t["bow_val"]))
    nwords = voc.info()["words"]
    ref = km.RefDatabase(nwords); db = pkg.KeyFrameDatabase(nwords)
    nkf = 5
    for i in range(nkf):                                           # frames 0..4 become keyframes, device to device
        assert db.add(fr, i, stream=st) == ref.add(vecs[i])
    for i in range(nkf):
        nb = [j for j in range(nkf) if j != i]
        db.set_covisibility(i, nb); ref.set_covisibility(i, nb)
    exp = [ref.DetectRelocalizationCandidates(v) for v in vecs]
    assert sum(len(e[0]) for e in exp) >= B
    d_cand = torch.full((B, 8), -1, dtype=torch.int32, device="cuda"); d_nc = torch.zeros(B, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    db.detect_relocalization_batch_device(fr, B, d_cand.data_ptr(), 8, d_nc.data_ptr(), st)
    stream.synchronize()
    nc = d_nc.cpu().numpy(); cand = d_cand.cpu().numpy()
    assert [cand[i, :nc[i]].tolist() for i in range(B)] == [e[0] for e in exp]
    assert db.reloc_scores().tobytes() == ref.reloc_scores().tobytes()
    # the per-call frame forms on the same resident frames
    for i in (5, 6, 7):
        c, wds, s = db.DetectRelocalizationCandidates(fr, index=i, stages=True)
        e = ref.DetectRelocalizationCandidates(vecs[i])
        assert c == e[0] and wds.tobytes() == e[1].tobytes() and s.tobytes() == e[2].tobytes()
        assert db.score(fr, list(range(nkf)), index=i).tobytes() == np.array(ref.score(vecs[i], range(nkf))).tobytes()


def _vec(rng, nwords, n, decades=3.0):
    ids = np.sort(rng.choice(nwords, n, replace=False)).astype(np.uint32)
    raw = 10.0 ** rng.uniform(-decades, 0, n)
    return ids, raw / raw.sum()


def _both(pkg, nwords):
    return km.RefDatabase(nwords), GpuImpl(pkg, nwords)


def _check_queries(ref, gpu, relocs=(), loops=()):
    out = []
    for q in relocs:
        e = ref.DetectRelocalizationCandidates(q); g = gpu.DetectRelocalizationCandidates(q)
        assert g[0] == e[0] and g[1].tobytes() == e[1].tobytes() and g[2].tobytes() == e[2].tobytes()
        assert gpu.reloc_scores().tobytes() == ref.reloc_scores().tobytes()
        out.append(e[0])
    for q, conn, ms in loops:
        e = ref.DetectLoopCandidates(q, conn, ms); g = gpu.DetectLoopCandidates(q, conn, ms)
        assert g[0] == e[0] and g[1].tobytes() == e[1].tobytes() and g[2].tobytes() == e[2].tobytes()
        out.append(e[0])
    return out


@pytest.mark.gpu
def test_gpu_edge_cases_small(pkg):
    rng = np.random.default_rng(11)
    ref, gpu = _both(pkg, NWORDS)
    q = _vec(rng, NWORDS, 300)
    empty = (np.zeros(0, np.uint32), np.zeros(0, np.float64))
    assert _check_queries(ref, gpu, [q, empty], [(q, [], 0.0)]) == [[], [], []]          # empty database
    assert len(gpu.db) == 0 and gpu.db.next_id() == 0
    sc = kfdb_scene.Scene(12, places=4, per_place=6, nwords=NWORDS)
    _scene_db(ref, sc); _scene_db(gpu, sc)
    r = _check_queries(ref, gpu, [sc.query(1)])
    assert r[0]
    before = gpu.reloc_scores().tobytes()
    far = (np.array([NWORDS - 1], np.uint32), np.array([1.0]))     # shares no word (id far above every base word is possible: checked below)
    assert all(NWORDS - 1 not in kf[0] for kf in sc.keyframes)
    assert _check_queries(ref, gpu, [empty, far], [(far, [], 0.0)]) == [[], [], []]
    assert gpu.reloc_scores().tobytes() == before                  # persistent scores untouched
    # a keyframe with a single word, found by a query that holds the word
    one = (np.array([NWORDS - 1], np.uint32), np.array([1.0]))
    i1 = ref.add(one); assert gpu.add(one) == i1
    assert _check_queries(ref, gpu, [far]) == [[i1]]
    assert gpu.score(far, [i1]).tobytes() == np.array(ref.score(far, [i1])).tobytes() and ref.score(far, [i1])[0] == 1.0
    # the capacity error carries the true count
    for _ in range(20):                                            # a view of two places, until the model returns several candidates
        q3 = sc.query(2, second=3)
        full = ref.DetectRelocalizationCandidates(q3)[0]
        assert gpu.db.DetectRelocalizationCandidates(q3) == full
        if len(full) >= 2:
            break
    assert len(full) >= 2
    ref.DetectRelocalizationCandidates(q3)
    with pytest.raises(pkg.OrbxError) as ei:
        gpu.db.DetectRelocalizationCandidates(q3, cap=1)
    assert ei.value.code == -2 and ei.value.ncand == len(ref.DetectRelocalizationCandidates(q3)[0])
    gpu.db.DetectRelocalizationCandidates(q3)                      # (the failed call scored like any other: keep the two in step)
    # every keyframe connected; min_score above every score
    everyone = list(range(ref.next_id()))
    assert _check_queries(ref, gpu, [], [(q3, everyone, 0.0), (q3, [], 2.0)]) == [[], []]
    with_low = _check_queries(ref, gpu, [], [(q3, [], 0.0)])
    assert with_low[0]
    # a neighbour list that names an erased id
    victim = sc.neighbours[full[0]][0]
    ref.erase(victim); gpu.erase(victim)
    _check_queries(ref, gpu, [sc.query(2), sc.query(2)], [(sc.query(2), [], 0.01)])
    assert len(gpu.db) == ref.next_id() - 1
    # malformed input
    for bad in ((np.array([5, 4], np.uint32), np.array([0.5, 0.5])), (np.array([NWORDS], np.uint32), np.array([1.0])),
                (np.array([1, 2], np.uint32), np.array([0.5, np.nan])), (np.array([1, 1], np.uint32), np.array([0.5, 0.5]))):
        for call in (lambda: gpu.db.add(bad), lambda: gpu.db.DetectRelocalizationCandidates(bad), lambda: gpu.db.score(bad, [0])):
            with pytest.raises(pkg.OrbxError) as ei:
                call()
            assert ei.value.code == -1
    for call in (lambda: gpu.db.erase(victim), lambda: gpu.db.score(q3, [victim]), lambda: gpu.db.set_covisibility(0, list(range(11)))):
        with pytest.raises(pkg.OrbxError) as ei:
            call()
        assert ei.value.code == -1


@pytest.mark.gpu
def test_gpu_equal_scores_keep_the_first(pkg):
    """identical keyframes score identically: the strict > of :192 / :316 keeps the group's own keyframe, then the first neighbour"""
    rng = np.random.default_rng(13)
    ref, gpu = _both(pkg, NWORDS)
    v = _vec(rng, NWORDS, 400); other = _vec(rng, NWORDS, 400)
    for bow in (v, v, other, v, v):
        assert gpu.add(bow) == ref.add(bow)
    for i, nb in enumerate([[1, 3, 4], [0, 3], [0, 1], [4, 0, 1], [3]]):
        ref.set_covisibility(i, nb); gpu.set_covisibility(i, nb)
    q = (v[0], v[1])
    r = _check_queries(ref, gpu, [q, q], [(q, [2], 0.5), (q, [0], 0.5)])
    # groups 0 and 3 reach the best accumulated score (their own + three equal neighbours); no neighbour ever replaces a group's keyframe
    assert r[0] == [0, 3] and r[1] == [0, 3] and r[2] == [0, 3] and r[3] == [3] and ref.stats["neighbour_best"] == 0


@pytest.mark.gpu
def test_gpu_long_vectors_and_large_vocabulary(pkg):
    """vectors longer than the kernels' 4096-word LDS tile on both sides, sparse ids in a vocabulary of ORBvoc's size"""
    nwords = 1000000
    rng = np.random.default_rng(17)
    ref, gpu = _both(pkg, nwords)
    pool = np.sort(rng.choice(nwords, 12000, replace=False))
    def sub(n):
        ids = np.sort(rng.choice(pool, n, replace=False)).astype(np.uint32)
        raw = 10.0 ** rng.uniform(-6, 0, n)
        return ids, raw / raw.sum()
    for n in (6000, 9000, 5000, 700, 4097, 8192, 4096):
        bow = sub(n)
        assert gpu.add(bow) == ref.add(bow)
    for i in range(7):
        nb = [(i + 1) % 7, (i + 3) % 7]
        ref.set_covisibility(i, nb); gpu.set_covisibility(i, nb)
    qs = [sub(9500), sub(5000), sub(4096), sub(300)]
    _check_queries(ref, gpu, qs, [(qs[0], [1], 0.1)])
    for q in qs:
        assert gpu.score(q, list(range(7))).tobytes() == np.array(ref.score(q, range(7))).tobytes()


@pytest.mark.gpu
def test_gpu_many_keyframes(pkg):
    """9000 keyframes (more than one launch's grid of 4 x 2048 waves: a wave takes several) with erased ones among them"""
    sc = kfdb_scene.Scene(19, places=225, per_place=40, nwords=NWORDS, base=120, extra=40, same=6, other=3)
    ref, gpu = _both(pkg, NWORDS)
    _scene_db(ref, sc); _scene_db(gpu, sc)
    for i in range(0, 9000, 17):
        ref.erase(i); gpu.erase(i)
    assert len(gpu.db) == 9000 - len(range(0, 9000, 17)) > 4 * 2048
    r = _check_queries(ref, gpu, [sc.query(3), sc.query(224), sc.query(3), sc.query(40, second=41)],
                       [(sc.query(224), list(range(8960, 8970)), 0.05), (sc.query(0), [], 0.0)])
    assert all(r) and ref.stats["stale_nonzero"] >= 1


@pytest.mark.gpu
def test_gpu_two_threads_one_handle(pkg):
    sc = kfdb_scene.Scene(23, nwords=NWORDS)
    ref, gpu = _both(pkg, NWORDS)
    _scene_db(ref, sc); _scene_db(gpu, sc)
    jobs = [[(sc.query(p), [p * 8, p * 8 + 1], 0.02) for p in ps] for ps in ((1, 2, 3, 4, 5, 6) * 3, (9, 8, 7, 6, 5, 4) * 3)]
    exp = [[(ref.DetectLoopCandidates(q, c, m)[0], ref.score(q, c)) for q, c, m in job] for job in jobs]
    got, errs = [None, None], []

    def work(k):
        try:
            got[k] = [(gpu.db.DetectLoopCandidates(q, c, m), gpu.db.score(q, c).tolist()) for q, c, m in jobs[k]]
        except Exception as e:               # surfaced below
            errs.append(e)
    ts = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in ts: t.start()
    for t in ts: t.join()
    assert not errs, errs
    assert got == exp and any(e[0] for e in exp[0])


@pytest.mark.gpu
def test_gpu_compiled_adapter(pkg, tmp_path):
    """adapter/KeyFrameDatabase.cc through tests/adapter_kfdb_driver.cc: both queries equal the transcription on the data the driver wrote"""
    import __graft_entry__ as ge
    ge.build()
    exe = os.path.join(str(tmp_path), "adapter_kfdb_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra"] + ADAPTER_INC +
                          [os.path.join(ROOT, "tests", "adapter_kfdb_driver.cc"), os.path.join(ROOT, "adapter", "KeyFrameDatabase.cc"),
                           "-L", os.path.join(ROOT, "orb-slam2_amd"), "-lorbx", "-lpthread", "-Wl,-rpath," + os.path.join(ROOT, "orb-slam2_amd"), "-o", exe])
    out = os.path.join(str(tmp_path), "kfdb.bin")
    r = subprocess.run([exe, out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    buf = open(out, "rb").read()
    pos = [0]

    def take(fmt):
        v = struct.unpack_from("<" + fmt, buf, pos[0]); pos[0] += struct.calcsize("<" + fmt)
        return v if len(v) > 1 else v[0]

    def take_vec():
        n = take("i")
        ids = np.frombuffer(buf, np.uint32, n, pos[0]); pos[0] += 4 * n
        vals = np.frombuffer(buf, np.float64, n, pos[0]); pos[0] += 8 * n
        return ids, vals

    def take_ints():
        n = take("i")
        v = np.frombuffer(buf, np.int32, n, pos[0]); pos[0] += 4 * n
        return [int(x) for x in v]

    nwords, nev = take("ii")
    ref = km.RefDatabase(nwords)
    id_of, nq = {}, 0                              # KeyFrame::mnId -> database id
    for _ in range(nev):
        kind = take("i")
        if kind == 0:                              # add
            mnid = take("i"); id_of[mnid] = ref.add(take_vec())
        elif kind == 1:                            # erase
            ref.erase(id_of.pop(take("i")))
        elif kind == 2:                            # the covisibility lists as they stand at a query
            mnid = take("i"); ref.set_covisibility(id_of[mnid], [id_of.get(m, -1) for m in take_ints()])
        elif kind == 3:                            # relocalisation query and the adaptor's answer (mnIds)
            q = take_vec(); got = take_ints()
            assert got == [k for c in ref.DetectRelocalizationCandidates(q)[0] for k, v in id_of.items() if v == c]
            nq += bool(got)
        elif kind == 4:
            q = take_vec(); conn = take_ints(); ms = take("f"); got = take_ints()
            exp = ref.DetectLoopCandidates(q, [id_of[m] for m in conn if m in id_of], ms)[0]
            assert got == [k for c in exp for k, v in id_of.items() if v == c]
            nq += bool(got)
        else:
            ref.clear(); id_of.clear()
    assert pos[0] == len(buf) and nq >= 4 and ref.stats["neighbour_best"] >= 1
