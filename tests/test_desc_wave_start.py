"""The start of a k_desc wave (grid decode, level search, the image's count row, the slot's packed keypoint, the patch address) and
the patch loads at the image edge, on the smallest shapes that reach every path of them: every result byte (keypoints 28 B, descriptors,
counts) against the CPU oracle.

  grids          batches of 1, 2, 7 (fewer than eight image columns: the divided blockIdx.x), 8 (exactly the eight columns) and 9 images
                 (two image groups, the second partial), 320x240, 8 levels, 500 features
  k_desc<16>     an extractor with 9 levels at 400x300
  count row      an image whose upper levels keep no keypoint, one with a single keypoint per level, a blank one (lc[l] == 0, total == 0, out_n)
  slots          a dense image under a quota of 100: levels end at or above their quota (j up to kp_cap - 1), asserted on the oracle
  reflect path   keypoints within 21 px of each of the four image edges, asserted on the oracle
  stale slots    one handle runs dense, blank, dense: each equals the oracle (= a fresh handle)
  row pass       an extractor created under ORBX_DESC_VALU_ROWPASS=1 gives the same bytes
  row-table wave one stereo pair through stereo_match_batch_device with ROWTAB_OF_EXTRACTION (slot "-1" shares the kernel's entry)
"""
import os

import numpy as np
import pytest

from tools import synth

pytestmark = pytest.mark.gpu

W, H = 320, 240
CFG = (500, 1.2, 8, 20, 7)
BF, MIN_Z = 386.1448, 386.1448 / 718.856


def _noise(seed, w, h, block=3):
    rng = np.random.Generator(np.random.PCG64(seed))
    t = rng.integers(0, 256, ((h + block - 1) // block, (w + block - 1) // block)).astype(np.uint8)
    return np.repeat(np.repeat(t, block, 0), block, 1)[:h, :w].copy()


def _blank():
    return np.full((H, W), 90, np.uint8)


def _strip():        # texture in a 16-px band: the levels from 5 up keep nothing
    img = _blank(); img[24:40, 24:296] = _noise(3, 272, 16, block=2)
    return img


def _window():       # a 12-px window: one keypoint on each of the lower levels
    img = _blank(); img[30:42, 30:42] = _noise(9, 12, 12)
    return img


def _same(tag, got, exp):
    (k, d), (ek, ed) = got, exp
    assert len(k) == len(ek), f"{tag}: {len(k)} keypoints vs oracle {len(ek)}"
    if k.tobytes() != ek.tobytes():
        for f in ek.dtype.names:
            bad = np.nonzero(k[f].view(np.uint32) != ek[f].view(np.uint32))[0]
            assert len(bad) == 0, f"{tag}: keypoint field {f} differs at {bad[:5].tolist()}: {k[f][bad[:3]]} vs {ek[f][bad[:3]]}"
    bad = np.nonzero((d != ed).any(axis=1))[0]
    assert len(bad) == 0, f"{tag}: {len(bad)} of {len(ed)} descriptors differ, first {bad[:5].tolist()}"
    assert d.tobytes() == ed.tobytes()


@pytest.fixture(scope="module")
def nine(oracle):
    """nine distinct images (index 4 blank, 6 with empty upper levels) and their oracle results, shared by the tests below"""
    imgs = [synth.image(700 + i, W, H) for i in range(9)]
    imgs[4] = _blank(); imgs[6] = _strip()
    o = oracle.Oracle(*CFG)
    return imgs, [o.extract(im) for im in imgs]


@pytest.mark.parametrize("B", [1, 2, 7, 8, 9])
def test_grids(pkg, nine, B):
    imgs, exp = nine
    ex = pkg.ORBextractor(*CFG, device=0, max_size=(W, H), max_batch=B)
    sel = [(3 * i + B) % 9 for i in range(B)]       # a different image order per batch size
    got = ex.extract_batch([imgs[s] for s in sel])
    for i, s in enumerate(sel):
        _same(f"B={B} image {i} (#{s})", got[i], exp[s])
    assert ex.debug_launch_forms()["desc_levels"] == 8


def test_nine_levels(pkg, oracle):
    cfg = (500, 1.2, 9, 20, 7)
    imgs = [synth.image(722 + i, 400, 300) for i in range(3)]
    o = oracle.Oracle(*cfg)
    exp = [o.extract(im) for im in imgs]
    assert all((e[0]["octave"] == 8).any() for e in exp)
    ex = pkg.ORBextractor(*cfg, device=0, max_size=(400, 300), max_batch=3)
    got = ex.extract_batch(imgs)
    for i in range(3):
        _same(f"9 levels image {i}", got[i], exp[i])
    assert ex.debug_launch_forms()["desc_levels"] == 16
    _same("9 levels single", ex(imgs[1]), exp[1])


def test_empty_levels_and_blank(pkg, oracle):
    o = oracle.Oracle(*CFG)
    imgs = [_strip(), _blank(), _window(), synth.image(731, W, H)]
    exp = [o.extract(im) for im in imgs]
    per_level = [np.bincount(e[0]["octave"], minlength=8) for e in exp]
    assert per_level[0][:4].min() > 10 and per_level[0][5:].sum() == 0      # upper levels empty, lower ones full
    assert len(exp[1][0]) == 0                                              # nothing at all
    assert 0 < len(exp[2][0]) <= 8 and per_level[2].max() == 1 and per_level[2].min() == 0
    ex = pkg.ORBextractor(*CFG, device=0, max_size=(W, H), max_batch=4)
    got = ex.extract_batch(imgs)
    for i in range(4):
        _same(f"empty levels image {i}", got[i], exp[i])
    for i in (1, 0, 2):
        _same(f"empty levels single {i}", ex(imgs[i]), exp[i])


def test_levels_at_and_above_quota(pkg, oracle):
    cfg = (100, 1.2, 8, 20, 7)
    img = _noise(5, W, H)
    o = oracle.Oracle(*cfg)
    exp = o.extract(img)
    per_level = np.bincount(exp[0]["octave"], minlength=8)
    quota = np.asarray(o.features_per_level())
    assert (per_level >= quota).all() and (per_level > quota).any(), (per_level, quota)
    ex = pkg.ORBextractor(*cfg, device=0, max_size=(W, H), max_batch=2)
    _same("quota 100", ex(img), exp)
    got = ex.extract_batch([img, img[::-1].copy()])
    _same("quota 100 batch", got[0], exp)
    _same("quota 100 batch, flipped", got[1], o.extract(img[::-1].copy()))


def test_reflect_path_at_every_edge(pkg, oracle):
    img = _noise(5, W, H)
    o = oracle.Oracle(*CFG)
    ek, ed = o.extract(img)
    sf = np.asarray(o.scale_factors())
    lvl = ek["octave"]
    lw = np.array([int(np.rint(np.float32(W) * np.float32(1.0 / s))) for s in sf])[lvl]
    lh = np.array([int(np.rint(np.float32(H) * np.float32(1.0 / s))) for s in sf])[lvl]
    xl, yl = np.rint(ek["x"] / sf[lvl]), np.rint(ek["y"] / sf[lvl])
    near = [(xl < 21).sum(), (yl < 21).sum(), (xl + 21 >= lw).sum(), (yl + 21 >= lh).sum()]
    assert min(near) >= 1, near
    ex = pkg.ORBextractor(*CFG, device=0, max_size=(W, H))
    _same("reflect", ex(img), (ek, ed))


def test_stale_slots(pkg, oracle):
    o = oracle.Oracle(*CFG)
    dense, blank = _noise(11, W, H), _blank()
    e_dense, e_blank = o.extract(dense), o.extract(blank)
    assert len(e_dense[0]) >= 500 and len(e_blank[0]) == 0
    ex = pkg.ORBextractor(*CFG, device=0, max_size=(W, H), max_batch=2)
    _same("dense 1", ex(dense), e_dense)
    _same("blank", ex(blank), e_blank)
    _same("dense 2", ex(dense), e_dense)
    got = ex.extract_batch([blank, dense])
    _same("batch blank", got[0], e_blank)
    _same("batch dense", got[1], e_dense)
    _same("fresh handle", pkg.ORBextractor(*CFG, device=0, max_size=(W, H))(dense), e_dense)


def test_valu_row_pass_form(pkg, nine):
    imgs, exp = nine
    old = os.environ.get("ORBX_DESC_VALU_ROWPASS")
    os.environ["ORBX_DESC_VALU_ROWPASS"] = "1"
    try:
        ex = pkg.ORBextractor(*CFG, device=0, max_size=(W, H), max_batch=9)
    finally:
        if old is None:
            del os.environ["ORBX_DESC_VALU_ROWPASS"]
        else:
            os.environ["ORBX_DESC_VALU_ROWPASS"] = old
    got = ex.extract_batch(imgs)
    assert ex.debug_launch_forms()["desc_rowpass"] == 1
    for i in range(9):
        _same(f"VALU row pass image {i}", got[i], exp[i])
    ex2 = pkg.ORBextractor(*CFG, device=0, max_size=(W, H), max_batch=9)
    got2 = ex2.extract_batch(imgs[:3])
    assert ex2.debug_launch_forms()["desc_rowpass"] == 2
    for i in range(3):
        _same(f"matrix row pass image {i}", got2[i], exp[i])


def test_stereo_pair_with_row_table_of_extraction(pkg, oracle):
    import torch
    l, r = synth.stereo_pair(741, W, H)[:2]
    oL, oR = oracle.Oracle(*CFG), oracle.Oracle(*CFG)
    kL, dL = oL.extract(l); kR, dR = oR.extract(r)
    our, odp = oracle.stereo_match(oL, oR, kL, dL, kR, dR, BF, MIN_Z)
    assert (our >= 0).sum() > 50
    dev = torch.device("cuda", 0)
    imgs = torch.from_numpy(np.stack([l, r])).to(dev)
    ex = pkg.ORBextractor(*CFG, device=0, max_size=(W, H), max_batch=2)
    cap = ex.max_keypoints(W, H)
    kps = torch.zeros((2, cap, 7), dtype=torch.float32, device=dev)
    desc = torch.zeros((2, cap, 32), dtype=torch.uint8, device=dev)
    nout = torch.zeros(2, dtype=torch.int32, device=dev)
    ur = torch.full((1, cap), 123.0, dtype=torch.float32, device=dev)
    dp = torch.full((1, cap), 123.0, dtype=torch.float32, device=dev)
    for rep in range(2):
        ex.extract_batch_device(imgs.data_ptr(), H * W, W, 2, W, H, kps.data_ptr(), desc.data_ptr(), cap, nout.data_ptr(), None)
        assert pkg.orbx.stereo_row_table_available(ex, kps[1:].data_ptr(), 1, 1, cap)
        pkg.orbx.stereo_match_batch_device(ex, 0, ex, 1, 1, kps.data_ptr(), desc.data_ptr(), nout.data_ptr(),
                                           kps[1:].data_ptr(), desc[1:].data_ptr(), nout[1:].data_ptr(), cap,
                                           BF, MIN_Z, ur.data_ptr(), dp.data_ptr(), None, row_table=pkg.orbx.ROWTAB_OF_EXTRACTION)
        ex.sync()
        n = nout.cpu().numpy()
        k = kps.cpu().numpy().view(np.uint8).reshape(2, cap, 28)
        d = desc.cpu().numpy()
        assert int(n[0]) == len(kL) and int(n[1]) == len(kR)
        assert k[0, :n[0]].tobytes() == kL.tobytes() and d[0, :n[0]].tobytes() == dL.tobytes(), f"rep {rep}: left eye differs"
        assert k[1, :n[1]].tobytes() == kR.tobytes() and d[1, :n[1]].tobytes() == dR.tobytes(), f"rep {rep}: right eye differs"
        assert ur.cpu().numpy()[0, :n[0]].tobytes() == our.tobytes(), f"rep {rep}: uRight differs"
        assert dp.cpu().numpy()[0, :n[0]].tobytes() == odp.tobytes(), f"rep {rep}: depth differs"
