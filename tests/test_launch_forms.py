"""Parity of every launch form that batch size and image geometry select, each against the CPU oracle byte for byte.

The host code picks kernel instances and grids by how many images a launch holds and by the geometry (the extractor's stages, each
in its own file: orbx_pyramid_launch, orbx_fast_launch, orbx_tree_launch, orbx_desc_launch in orbx_pyramid.hip / orbx_fast.hip /
orbx_tree.hip / orbx_desc.hip; orbx_stereo.hip: orbx_stereo_match_batch_device, orbx_bow.hip: bow_launch).  Each case below
asserts through orbx_debug_launch_forms / orbx_debug_bow_last_form that the form it targets really ran, so a change of a
threshold cannot leave a case silently testing something else.

  decision                 case
  pyramid regime 0/1/2     test_headline_batches (B = 256 / 150: 0, B = 1: 2), test_sixteen_levels_batches (0, 1, 2 at 16 levels)
  FAST waves, grid order   test_headline_batches (1 wave image-major, > 1 wave for B = 1), test_4096_square (cell-major 1-wave grid)
  quadtree threads         test_headline_batches, test_tree256_storage (65 images: 256, 64 images: 1024)
  quadtree tables          test_tree256_storage[640x480_hbm] (HBM tables with 256 threads), the others: LDS
  points per (image, lvl)  test_tree256_storage: registers (<= 3072), + LDS overflow (<= 4096), HBM scratch (> 4096) at 1241x376;
                           LDS arrays (<= 5120) and HBM scratch (> 5120) at 1024x768
  k_desc <8> / <16>        test_headline_batches (<8>, 2 and 300 / 512 images), test_sixteen_levels_batches (<16>, 33 images)
  k_stereo                 test_headline_batches: B = 1 folded (1 keypoint per wave), B = 256 two full XCD groups of 128 pairs,
                           B = 150 a full and a partial group
  k_bow2                   test_bow_throughput_forms: table form on the XCD keyframe grid, dense rows and compact lists
"""
import hashlib
import os
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tools import synth

W, H, NF = 1241, 376, 1000
BF, MIN_Z = 386.1448, 386.1448 / 718.856     # Examples/Stereo/KITTI00-02.yaml:8,25
PITCH = (W + 63) // 64 * 64


def _workers():
    """oracle threads: OMP_NUM_THREADS (the CPU share of the machine) capped at 16 and at the affinity mask"""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = 1
    env = os.environ.get("OMP_NUM_THREADS", "")
    if env.isdigit() and int(env) > 0:
        n = min(n, int(env))
    return max(1, min(n, 16))


def _pmap(fn, items):
    with ThreadPoolExecutor(_workers()) as pool:
        return list(pool.map(fn, items))


def _oracle_map(oracle, cfg, fn, items):
    """fn((oracle_a, oracle_b), item) on a thread pool, one pair of Oracle instances per thread (an instance is not shareable:
    it keeps the pyramid of its last image, which stereo_match reads)"""
    local = threading.local()

    def run(item):
        if not hasattr(local, "o"):
            local.o = (oracle.Oracle(*cfg), oracle.Oracle(*cfg))
        return fn(local.o, item)
    return _pmap(run, items)


def _noise(seed, w, h, block=3):
    rng = np.random.Generator(np.random.PCG64(seed))
    t = rng.integers(0, 256, ((h + block - 1) // block, (w + block - 1) // block)).astype(np.uint8)
    return np.repeat(np.repeat(t, block, 0), block, 1)[:h, :w].copy()


def _digest(*arrays):
    h = hashlib.sha1()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.digest()


def _cmp_image(tag, i, n, k, d, ek, ed):
    """keypoint records of image i against the oracle, naming the first field that differs"""
    assert n == len(ek), f"{tag} image {i}: {n} keypoints vs oracle {len(ek)}"
    if k[:n].tobytes() != ek.tobytes():
        got = np.frombuffer(k[:n].tobytes(), dtype=ek.dtype)
        for f in ek.dtype.names:
            bad = np.nonzero(got[f].view(np.uint32) != ek[f].view(np.uint32))[0]
            assert len(bad) == 0, f"{tag} image {i}: keypoint field {f} differs at {bad[:5].tolist()}: {got[f][bad[:3]]} vs {ek[f][bad[:3]]}"
        raise AssertionError(f"{tag} image {i}: keypoint records differ")
    bad = np.nonzero((d[:n] != ed).any(axis=1))[0]
    assert len(bad) == 0, f"{tag} image {i}: {len(bad)} descriptors differ, first {bad[:5].tolist()}"


def _assert_forms(tag, got, **want):
    bad = {k: (got[k], v) for k, v in want.items() if (got[k] not in v if isinstance(v, tuple) else got[k] != v)}
    assert not bad, f"{tag}: launch forms (got, wanted) {bad}; all: {got}"


# ------------------------------------------------------------------------------------------- (a) the headline step

SPECIAL = {0: "flat", 7: "left_window", 8: "dense", 63: "sparse", 64: "right_window", 127: "dense", 128: "sparse",
           129: "left_window", 255: "dense"}


def _headline_pairs():
    """256 distinct KITTI-shape pairs: 32 synth.stereo_pair bases, each slot a different horizontal roll of both eyes (and for some
    variants a vertical flip of both): rows stay epipolar.  SPECIAL slots: a featureless pair, pairs with one eye flat outside a
    window (unequal counts in one batch), pairs with a dense level 0 (> 4096 FAST candidates: a 300-px noise strip seen by both eyes
    20 px apart) and sparse pairs (<= 3072)"""
    nb = 32
    bases = _pmap(lambda i: synth.stereo_pair(4000 + i, W, H)[:2], range(nb))
    sparse = _pmap(lambda i: synth.stereo_pair(4100 + i, W, H, nshapes=500)[:2], range(2))
    pairs, n_sparse = [], 0
    for s in range(256):
        b, v = s % nb, s // nb
        l, r = bases[b]
        kind = SPECIAL.get(s)
        if kind == "sparse":
            l, r = sparse[n_sparse]; n_sparse += 1
        l, r = np.roll(l, 151 * v + 7 * b, axis=1), np.roll(r, 151 * v + 7 * b, axis=1)
        if v in (1, 4, 6):
            l, r = l[::-1], r[::-1]
        l, r = l.copy(), r.copy()
        if kind == "flat":
            l = np.full((H, W), 77, np.uint8); r = np.full((H, W), 77, np.uint8)
        elif kind == "left_window":
            l2 = np.full_like(l, 200); l2[100:200, 500:620] = l[100:200, 500:620]; l = l2
        elif kind == "right_window":
            r2 = np.full_like(r, 60); r2[100:200, 500:620] = r[100:200, 500:620]; r = r2
        elif kind == "dense":
            strip = _noise(4200 + s, 300, H)
            l[:, 400:700] = strip; r[:, 380:680] = strip
        pairs.append((l, r))
    return pairs


def _stereo_oracle(oracle, pairs):
    def one(o, lr):
        oL, oR = o
        kL, dL = oL.extract(lr[0]); kR, dR = oR.extract(lr[1])
        ur, dp = oracle.stereo_match(oL, oR, kL, dL, kR, dR, BF, MIN_Z)
        return kL, dL, kR, dR, ur, dp, len(oL.candidates(0)[0]), len(oR.candidates(0)[0])
    return _oracle_map(oracle, (NF, 1.2, 8, 20, 7), one, pairs)


@pytest.mark.gpu
def test_headline_batches(pkg, oracle):
    """the stereo1000 step as bench.py times it (bench.StereoRig: 2 x 256 images on one handle, then the batched stereo match) on 256
    distinct pairs whose 512 oracle outputs are pairwise distinct, so an image or pair index error of any period (the XCD remaps of
    k_desc, k_stereo and k_fast work in groups of 8 and 128) changes the result.  The same handle then runs B = 1, 150 and 256 again
    (a permutation of the same pairs): every image and pair of every launch is checked"""
    import torch
    import bench
    pairs = _headline_pairs()
    exp = _stereo_oracle(oracle, pairs)
    # every image's output differs from every other one's (the featureless pair's two eyes are both empty by construction)
    dig = {}
    for p, e in enumerate(exp):
        for eye, (k, d) in enumerate(((e[0], e[1]), (e[2], e[3]))):
            if SPECIAL.get(p) == "flat":
                assert len(k) == 0
                continue
            key = _digest(k, d)
            assert key not in dig, f"pair {p} eye {eye} has the same oracle output as {dig[key]}: the batch would hide index errors"
            dig[key] = (p, eye)
    assert len(dig) == 510
    cands = np.array([c for e in exp for c in e[6:8]])
    assert (cands <= 3072).sum() >= 2 and ((cands > 3072) & (cands <= 4096)).sum() >= 100 and (cands > 4096).sum() >= 3, \
        f"level-0 candidate buckets not covered: {np.sort(cands)[:4]} .. {np.sort(cands)[-4:]}"
    assert sum((e[4] >= 0).sum() > 50 for e in exp) >= 240          # matches really occur in nearly every pair

    dev = torch.device("cuda", 0)
    rig = bench.StereoRig(pkg, torch, dev, 0, W, H, NF, 256, pairs)
    cap = rig.cap

    def run(tag, order, imgs=None):
        B = len(order)
        if imgs is None:
            host = np.zeros((2 * B, H, PITCH), np.uint8)
            for i, p in enumerate(order):
                host[i, :, :W] = pairs[p][0]; host[B + i, :, :W] = pairs[p][1]
            imgs = torch.from_numpy(host).to(dev)
        for t, v in ((rig.ur, -777.0), (rig.dp, -777.0), (rig.kps, -3.0), (rig.nout, -1)):
            t.fill_(v)                                     # poisoned: everything the launch owns must be rewritten
        rig.desc.fill_(0xA5)
        torch.cuda.synchronize()
        rig.B = B                                          # the rig's own step(): the call sequence bench.py times, at batch B
        rig.step(imgs)
        rig.stream.synchronize()
        forms = rig.ex.debug_launch_forms()
        n = rig.nout.cpu().numpy()
        k = rig.kps.cpu().numpy().view(np.uint8).reshape(rig.kps.shape[0], cap, 28)
        d = rig.desc.cpu().numpy(); ur = rig.ur.cpu().numpy(); dp = rig.dp.cpu().numpy()
        for i, p in enumerate(order):
            kL, dL, kR, dR, our, odp = exp[p][:6]
            _cmp_image(f"{tag} pair {p} left", i, int(n[i]), k[i], d[i], kL, dL)
            _cmp_image(f"{tag} pair {p} right", B + i, int(n[B + i]), k[B + i], d[B + i], kR, dR)
            nl = len(kL)
            bad = np.nonzero(ur[i, :nl].view(np.uint32) != our.view(np.uint32))[0]
            assert len(bad) == 0, f"{tag} pair {p} (slot {i}): uRight differs at {bad[:5].tolist()}: {ur[i, bad[:5]]} vs {our[bad[:5]]}"
            bad = np.nonzero(dp[i, :nl].view(np.uint32) != odp.view(np.uint32))[0]
            assert len(bad) == 0, f"{tag} pair {p} (slot {i}): depth differs at {bad[:5].tolist()}: {dp[i, bad[:5]]} vs {odp[bad[:5]]}"
        return forms

    f = run("B=256", list(range(256)), rig.imgs)
    _assert_forms("B=256", f, pyramid_regime=0, fast_waves=1, fast_image_major=1, tree_threads=256, tree_tab_lds=1, tree_reg=1,
                  desc_levels=8, stereo_kpw=4, stereo_xcd_grid=1)
    perm = np.random.Generator(np.random.PCG64(5)).permutation(256).tolist()
    f = run("B=1", [8])                                                 # a dense pair through the 1024-thread tree
    _assert_forms("B=1", f, pyramid_regime=2, fast_waves=(2, 3, 4), tree_threads=1024, desc_levels=8, stereo_kpw=1, stereo_xcd_grid=0)
    f = run("B=150", perm[:150])
    _assert_forms("B=150", f, pyramid_regime=0, fast_waves=1, tree_threads=256, desc_levels=8, stereo_kpw=4, stereo_xcd_grid=1)
    f = run("B=256 permuted", perm)
    _assert_forms("B=256 permuted", f, pyramid_regime=0, tree_threads=256, stereo_kpw=4, stereo_xcd_grid=1)


# ------------------------------------------------------------------------------------------- (b) the quadtree's storage paths

def _mono_set(kind):
    """65 distinct images of one geometry and the level-0 candidate buckets they must cover; (w, h, nfeatures, images, buckets)"""
    def rolled(base, i):
        return np.roll(np.roll(base, 97 * i, axis=1), 31 * i, axis=0)
    if kind == "1241x376":
        w, h, nf = W, H, NF
        b = _pmap(lambda a: synth.image(*a), [(5000, w, h, 500), (5001, w, h, 1500), (5002, w, h, 3000)])
        dense = b[1].copy(); dense[:, 300:700] = _noise(5003, 400, h)
        bases = [b[0], b[1], b[2], dense]
        buckets = [(0, 3072), (3073, 4096), (4097, 1 << 30)]
    elif kind == "1024x768":
        w, h, nf = 1024, 768, NF
        b = _pmap(lambda a: synth.image(*a), [(5010, w, h, 1500), (5011, w, h, 3000)])
        dense = b[0].copy(); dense[:, 200:500] = _noise(5012, 300, h)
        bases = [b[0], b[1], dense]
        buckets = [(0, 5120), (5121, 1 << 30)]
    else:
        w, h, nf = 640, 480, 12000
        bases = _pmap(lambda a: synth.image(*a), [(5020, w, h, 1500), (5021, w, h, 3000)])
        buckets = [(0, 1 << 30)]
    imgs = [rolled(bases[i % len(bases)], i // len(bases)) for i in range(65)]
    return w, h, nf, imgs, buckets


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["1241x376", "1024x768", "640x480_hbm"])
def test_tree256_storage(pkg, oracle, kind):
    """k_tree with 256 threads (65 images of 8 levels: 520 workgroups > 512) and the 1024-thread form on 64 images of the same content:
    1241x376 keeps a level's points in registers (<= 3072), with an LDS overflow (<= 4096) or in the HBM scratch (more); 1024x768 keeps
    them in LDS arrays (<= 5120) or the HBM scratch; 640x480 at 12 000 features puts the node tables in HBM"""
    import torch
    w, h, nf, imgs, buckets = _mono_set(kind)

    def one(o, img):
        k, d = o[0].extract(img)
        return k, d, len(o[0].candidates(0)[0])
    exp = _oracle_map(oracle, (nf, 1.2, 8, 20, 7), one, imgs)
    assert len({_digest(e[0], e[1]) for e in exp}) == 65
    cands = np.array([e[2] for e in exp])
    for lo, hi in buckets:        # both batches hold images of every bucket: the case cannot go vacuous
        assert ((cands[:64] >= lo) & (cands[:64] <= hi)).sum() >= 3, f"{kind}: no level-0 candidate count in [{lo}, {hi}]: {sorted(cands)}"
    pitch = (w + 63) // 64 * 64
    host = np.zeros((65, h, pitch), np.uint8)
    for i, im in enumerate(imgs):
        host[i, :, :w] = im
    dev = torch.device("cuda", 0)
    d_img = torch.from_numpy(host).to(dev)
    ex = pkg.ORBextractor(nf, 1.2, 8, 20, 7, device=0, max_size=(w, h), max_batch=65)
    cap = ex.max_keypoints(w, h)
    kps = torch.zeros((65, cap, 7), dtype=torch.float32, device=dev)
    desc = torch.zeros((65, cap, 32), dtype=torch.uint8, device=dev)
    nout = torch.zeros(65, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(device=dev)
    for B, threads in ((65, 256), (64, 1024)):
        kps.fill_(-3.0); desc.fill_(0xA5); nout.fill_(-1)
        torch.cuda.synchronize()
        ex.extract_batch_device(d_img.data_ptr(), h * pitch, pitch, B, w, h, kps.data_ptr(), desc.data_ptr(), cap, nout.data_ptr(), stream.cuda_stream)
        ex.sync(stream.cuda_stream)
        f = ex.debug_launch_forms()
        _assert_forms(f"{kind} B={B}", f, tree_threads=threads, tree_tab_lds=int(kind != "640x480_hbm"), tree_reg=int(kind == "1241x376"),
                      desc_levels=8)
        n = nout.cpu().numpy(); k = kps.cpu().numpy().view(np.uint8).reshape(65, cap, 28); d = desc.cpu().numpy()
        for i in range(B):
            _cmp_image(f"{kind} B={B}", i, int(n[i]), k[i], d[i], exp[i][0], exp[i][1])


# ------------------------------------------------------------------------------------------- (c) BoW throughput forms

@pytest.mark.gpu
def test_bow_throughput_forms(pkg, oracle):
    """the euroc_bow step's search: 28 extracted 752x480 frames against 150 keyframes derived as bench.py derives its map (one full
    128-keyframe XCD group and a partial one); the dense search in the automatic form (4200 pairs: the table form) and the compact
    search (bench.py's default) with a capacity of every feature and with a small capacity that cuts the lists"""
    import torch
    w, h, B, NKF = 752, 480, 28, 150
    pitch = 768
    bases = _pmap(lambda s: synth.image(s, w, h), range(6000, 6007))
    imgs = [np.roll(bases[i % 7], 53 * (i // 7), axis=1) for i in range(B)]
    imgs[5] = np.full((h, w), 90, np.uint8)                  # a featureless frame inside the batch
    host = np.zeros((B, h, pitch), np.uint8)
    for i in range(B):
        host[i, :, :w] = imgs[i]
    dev = torch.device("cuda", 0)
    d_img = torch.from_numpy(host).to(dev)
    ex = pkg.ORBextractor(NF, 1.2, 8, 20, 7, device=0, max_size=(w, h), max_batch=B)
    cap = ex.max_keypoints(w, h)
    d_kps = torch.zeros((B, cap, 7), device=dev); d_desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device=dev)
    d_n = torch.zeros(B, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(device=dev); st = stream.cuda_stream
    ex.extract_batch_device(d_img.data_ptr(), h * pitch, pitch, B, w, h, d_kps.data_ptr(), d_desc.data_ptr(), cap, d_n.data_ptr(), st)
    stream.synchronize()
    n = d_n.cpu().numpy(); desc = d_desc.cpu().numpy(); kps = d_kps.cpu().numpy().view(np.uint8).reshape(B, cap, 28)
    oex = _oracle_map(oracle, (NF, 1.2, 8, 20, 7), lambda o, im: o[0].extract(im), imgs)
    for i in range(B):
        _cmp_image("bow frames", i, int(n[i]), kps[i], desc[i], oex[i][0], oex[i][1])
    assert n[5] == 0
    rng = np.random.Generator(np.random.PCG64(77))
    par, leaf, nd, wt = synth.vocab_tree(78, 10, 4, stop_frac=0.02, data=desc[0, :n[0]])
    voc = pkg.ORBVocabulary(10, 4, par, leaf, nd, wt); ovoc = oracle.Vocabulary(10, 4, par, leaf, nd, wt)
    frames = []
    for i in range(B):
        t = ovoc.transform(desc[i, :n[i]], 4)
        frames.append(dict(desc=desc[i, :n[i]], node_id=t["fv_node_id"], node_off=t["fv_node_off"], feat=t["fv_feat"],
                           flag=np.zeros(n[i], np.uint8), angle=oex[i][0]["angle"].copy()))
    kfs = []
    for j in range(NKF):             # bench.py: keyframe = a frame's descriptors with Bernoulli(0.08) bit flips, shuffled; hasGoodMP ~ 0.6
        base = frames[j % 3]
        perm = rng.permutation(len(base["desc"]))
        dk = synth.flip_bits(rng, base["desc"], 0.08)[perm]
        t = ovoc.transform(dk, 4)
        kfs.append(dict(desc=dk, node_id=t["fv_node_id"], node_off=t["fv_node_off"], feat=t["fv_feat"],
                        flag=(rng.random(len(dk)) < 0.6).astype(np.uint8), angle=base["angle"][perm]))
    expect = _pmap(lambda ij: oracle.search_by_bow_kf_f(kfs[ij[1]], frames[ij[0]], 0.75, True), [(i, j) for i in range(B) for j in range(NKF)])
    expect = [expect[i * NKF:(i + 1) * NKF] for i in range(B)]
    assert sum(en for row in expect for _, en in row) > 20 * NKF * B
    db = pkg.BowDatabase(kfs)
    fr = pkg.BowFrames(B, cap)
    fr.transform(voc, d_kps.data_ptr(), d_desc.data_ptr(), d_n.data_ptr(), B, 4, st)
    d_nm = torch.zeros((B, NKF), dtype=torch.int32, device=dev)
    d_match = torch.full((B, NKF, cap), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    pkg.orbx.debug_set_bow_form("auto")
    fr.search(db, B, d_match.data_ptr(), d_nm.data_ptr(), 0.75, True, st)
    stream.synchronize()
    assert pkg.orbx.debug_bow_last_form() == dict(form="table", xcd_grid=True, compact=False)
    m = d_match.cpu().numpy(); nm = d_nm.cpu().numpy()
    for i in range(B):
        for j in range(NKF):
            e, en = expect[i][j]
            assert nm[i, j] == en, f"dense: frame {i} keyframe {j}: {nm[i, j]} matches vs oracle {en}"
            bad = np.nonzero(m[i, j, :n[i]] != e)[0]
            assert len(bad) == 0, f"dense: frame {i} keyframe {j}: match row differs at {bad[:5].tolist()}"
    for cap_pairs in (cap, 24):
        d_pairs = torch.full((B, NKF, cap_pairs, 2), -7, dtype=torch.int32, device=dev)
        d_nm.fill_(-1)
        torch.cuda.synchronize()
        fr.search_compact(db, B, d_pairs.data_ptr(), cap_pairs, d_nm.data_ptr(), 0.75, True, st)
        stream.synchronize()
        assert pkg.orbx.debug_bow_last_form() == dict(form="table", xcd_grid=True, compact=True)
        lst = d_pairs.cpu().numpy(); nm = d_nm.cpu().numpy()
        cut = 0
        for i in range(B):
            for j in range(NKF):
                e, en = expect[i][j]
                slots = np.nonzero(e >= 0)[0]
                want = np.stack([slots, e[slots]], axis=1).astype(np.int32)[:cap_pairs]   # the first cap_pairs matches in frame-feature order
                assert nm[i, j] == en == len(slots), f"compact cap={cap_pairs}: frame {i} keyframe {j}: count {nm[i, j]} vs oracle {en}"
                got = lst[i, j, :len(want)]
                assert (got == want).all(), f"compact cap={cap_pairs}: frame {i} keyframe {j}: list differs at {np.nonzero((got != want).any(1))[0][:5].tolist()}"
                assert (lst[i, j, len(want):] == -7).all(), f"compact cap={cap_pairs}: frame {i} keyframe {j}: written beyond the list"
                cut += en > cap_pairs
        if cap_pairs == 24:
            assert cut > NKF, "the small capacity cut too few lists"


# ------------------------------------------------------------------------------------------- (d) geometry limits

@pytest.mark.gpu
def test_sixteen_levels_batches(pkg, oracle):
    """16 levels at scale factor 1.1: k_desc<16>; 33 images (528 workgroups: the 256-thread tree, one launch per pyramid level), 20 images
    (per-level launches for the big levels, grouped launches for the small ones) and 8 images (every k_pyr_group group, the third and
    fourth included)"""
    import torch
    w, h, nf, sf, nl = 640, 480, 1000, 1.1, 16
    bases = _pmap(lambda s: synth.image(s, w, h), range(7000, 7011))
    imgs = [np.roll(bases[i % 11], 71 * (i // 11), axis=1) for i in range(33)]
    exp = _oracle_map(oracle, (nf, sf, nl, 20, 7), lambda o, im: o[0].extract(im), imgs)
    assert len({_digest(*e) for e in exp}) == 33
    pitch = 640
    dev = torch.device("cuda", 0)
    d_img = torch.from_numpy(np.stack(imgs)).to(dev)
    ex = pkg.ORBextractor(nf, sf, nl, 20, 7, device=0, max_size=(w, h), max_batch=33)
    cap = ex.max_keypoints(w, h)
    kps = torch.zeros((33, cap, 7), dtype=torch.float32, device=dev)
    desc = torch.zeros((33, cap, 32), dtype=torch.uint8, device=dev)
    nout = torch.zeros(33, dtype=torch.int32, device=dev)
    regimes = set()
    for B, threads in ((33, 256), (20, 1024), (8, 1024)):
        kps.fill_(-3.0); desc.fill_(0xA5); nout.fill_(-1)
        torch.cuda.synchronize()
        ex.extract_batch_device(d_img.data_ptr(), h * pitch, pitch, B, w, h, kps.data_ptr(), desc.data_ptr(), cap, nout.data_ptr(), None)
        ex.sync()
        f = ex.debug_launch_forms()
        _assert_forms(f"16 levels B={B}", f, tree_threads=threads, desc_levels=16)
        regimes.add(f["pyramid_regime"])
        n = nout.cpu().numpy(); k = kps.cpu().numpy().view(np.uint8).reshape(33, cap, 28); d = desc.cpu().numpy()
        for i in range(B):
            _cmp_image(f"16 levels B={B}", i, int(n[i]), k[i], d[i], exp[i][0], exp[i][1])
    assert regimes == {0, 1, 2}, regimes


def _tiled_4096(seed):
    """4096 x 4096 from 16 flipped / transposed copies of one 1024 x 1024 synth.image (synth at full size is slow)"""
    t = synth.image(seed, 1024, 1024, nshapes=2000)
    rows = []
    for r in range(4):
        row = []
        for c in range(4):
            v = (r * 4 + c) % 8
            x = t.T if v & 4 else t
            x = x[::-1] if v & 1 else x
            x = x[:, ::-1] if v & 2 else x
            row.append(x)
        rows.append(np.concatenate(row, axis=1))
    return np.ascontiguousarray(np.concatenate(rows, axis=0))


@pytest.mark.gpu
def test_4096_square(pkg, oracle):
    """the documented 4096-px limit (12-bit packed coordinates) at (1.2, 8) and (1.1, 16); the second has more than 65 535 FAST cells,
    which selects the cell-major one-wave k_fast grid.  A 4097-px side is refused."""
    img = _tiled_4096(8000)
    cfgs = [(2000, 1.2, 8), (2000, 1.1, 16)]

    def one(cfg):
        o = oracle.Oracle(cfg[0], cfg[1], cfg[2], 20, 7)
        return o.extract(img)
    exp = _pmap(one, cfgs)
    for (nf, sf, nl), (ek, ed) in zip(cfgs, exp):
        ex = pkg.ORBextractor(nf, sf, nl, 20, 7, device=0, max_size=(4096, 4096))
        k, d = ex(img)
        tag = f"4096x4096 sf={sf} levels={nl}"
        f = ex.debug_launch_forms()
        if nl == 16:
            _assert_forms(tag, f, fast_waves=1, fast_image_major=0, desc_levels=16)
        assert len(ek) > nf // 2 and (ek["x"] > 4000).any() and (ek["y"] > 4000).any(), tag
        _cmp_image(tag, 0, len(k), k.view(np.uint8).reshape(len(k), 28), d, ek, ed)
    for w, h in ((4097, 64), (64, 4097)):
        ex = pkg.ORBextractor(500, 1.2, 4, 20, 7, device=0, max_size=(w, h))
        with pytest.raises(pkg.OrbxError):
            ex(np.zeros((h, w), np.uint8))
