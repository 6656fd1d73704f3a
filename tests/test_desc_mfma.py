"""k_desc's row pass on the matrix cores (nine v_mfma_i32_16x16x64_i8 per keypoint, orbx_desc.hip) against the CPU oracle, byte for byte,
on the smallest inputs at which it can go wrong, and against the vector-ALU row pass it replaced (ORBX_DESC_VALU_ROWPASS=1 when the
extractor is created), which stays as a second instantiation of the kernel.

  what can go wrong                                   case
  M/N lane mapping transposed, D layout swapped       test_layout_probe: a bright column, a bright row, a left-to-right ramp beside a keypoint
  u16 packing / clamp at the top of the range         test_saturation: 0 / 255 blocks, row sums 255 * 257 = 65 535
  accumulator start (128 * sum of the taps)           both tap profiles in every oracle case (sums 257 and 256)
  reflect path with the 48-byte raw pitch             test_border_keypoints: keypoints within 21 px of all four edges on four levels
  alignment assumed of the SOURCE, not of the LDS     test_odd_pitch_and_base: level 0 at an odd address with an odd pitch
  the two forms disagree, either grid                 test_forms_agree: one 320 x 240 image (under-eight grid) and a batch of 9 (eight-wide grid)
"""
import numpy as np
import pytest

from tools import synth

pytestmark = pytest.mark.gpu


def _oracle(oracle, cfg, img, profile):
    o = oracle.Oracle(*cfg)
    o.set_cv_profile(profile)
    return o.extract(img)


def _same(tag, got, want):
    (k, d), (ok, od) = got, want
    assert len(k) == len(ok), f"{tag}: {len(k)} keypoints, oracle {len(ok)}"
    assert k.tobytes() == ok.tobytes(), f"{tag}: keypoints differ from the oracle"
    bad = np.flatnonzero((d != od).any(axis=1))
    assert bad.size == 0, f"{tag}: {bad.size} of {len(d)} descriptors differ from the oracle, first at {bad[:5]}"


def _both_profiles(pkg, oracle, tag, cfg, img, min_kps):
    h, w = img.shape
    ex = pkg.ORBextractor(*cfg, device=0, max_size=(w, h))
    out = []
    for profile in (pkg.orbx.CV_PROFILE_3_2, pkg.orbx.CV_PROFILE_3_4_2):
        ex.set_cv_profile(profile)
        got = ex(img)
        assert ex.debug_launch_forms()["desc_rowpass"] == 2, "the matrix-core form did not run"
        want = _oracle(oracle, cfg, img, profile)
        assert len(want[0]) >= min_kps, (tag, len(want[0]))
        _same(f"{tag}, profile {profile}", got, want)
        out.append(got)
    return out


def _probe_image():
    """96 x 96, four 3 x 3 dots; beside three of them, inside the keypoint's 31-px patch: one bright column, one bright row, a ramp"""
    img = np.full((96, 96), 40, np.uint8)
    for x, y in ((30, 30), (66, 30), (30, 66), (66, 66)):
        synth._put_dot(img, x, y, True)
    img[22:39, 37] = 230
    img[37, 58:75] = 230
    img[58:75, 35:43] = (70 + 22 * np.arange(8)).astype(np.uint8)[None, :]
    return img


def test_layout_probe(pkg, oracle):
    cfg = (500, 1.2, 2, 20, 7)
    img = _probe_image()
    (k, d), (k1, d1) = _both_profiles(pkg, oracle, "probe", cfg, img, 8)
    lvl0 = {(float(a["x"]), float(a["y"])) for a in k if a["octave"] == 0}
    assert {(30.0, 30.0), (66.0, 30.0), (30.0, 66.0), (66.0, 66.0)} <= lvl0, lvl0      # the dots beside the patterns are kept, on the interior path
    # (the steered descriptor of the column keypoint equals that of the row keypoint -- one is the other rotated by 90 degrees -- so the
    # patterns are told apart by the oracle comparison above, where a transposed row pass blurs a mirrored patch under an unmirrored angle)
    assert (d != d1).any(), "the two tap profiles gave the same descriptors: the test image does not tell them apart"


def test_saturation(pkg, oracle):
    img = synth.block_checkerboard(w=160, h=120)
    img = img[0] if isinstance(img, tuple) else img
    assert img.min() == 0 and img.max() == 255
    _both_profiles(pkg, oracle, "0/255 blocks", (300, 1.2, 2, 20, 7), img, 5)


def test_border_keypoints(pkg, oracle):
    cfg = (500, 1.2, 4, 20, 7)
    img = synth.border_lattice()
    (k, d), _ = _both_profiles(pkg, oracle, "border lattice", cfg, img, 50)
    s = np.float64(np.float32(1.2)) ** k["octave"]
    lx, ly = k["x"] / s, k["y"] / s
    for l in range(4):
        m = k["octave"] == l
        w, h = int(round(320 / 1.2 ** l)), int(round(240 / 1.2 ** l))
        near = [(lx[m] < 20.5).sum(), (lx[m] + 21.5 >= w).sum(), (ly[m] < 20.5).sum(), (ly[m] + 21.5 >= h).sum()]
        assert min(near) >= 1, f"level {l}: keypoints within 21 px of (left, right, top, bottom) = {near}"


def test_odd_pitch_and_base(pkg, oracle):
    import torch
    W, H, pitch, base = 320, 240, 333, 3
    cfg = (500, 1.2, 4, 20, 7)
    img = synth.image(5, W, H)
    host = np.full(base + H * pitch + 64, 0xA5, np.uint8)
    host[base:base + H * pitch].reshape(H, pitch)[:, :W] = img
    dev = torch.device("cuda", 0)
    buf = torch.from_numpy(host).to(dev)
    ex = pkg.ORBextractor(*cfg, device=0, max_size=(W, H))
    cap = ex.max_keypoints(W, H)
    kps = torch.zeros((cap, 7), dtype=torch.float32, device=dev)
    desc = torch.zeros((cap, 32), dtype=torch.uint8, device=dev)
    nout = torch.zeros((1,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    assert (buf.data_ptr() + base) % 2 == 1 and pitch % 2 == 1
    ex.extract_batch_device(buf.data_ptr() + base, H * pitch, pitch, 1, W, H, kps.data_ptr(), desc.data_ptr(), cap, nout.data_ptr(), None)
    ex.sync()
    assert ex.debug_launch_forms()["desc_rowpass"] == 2
    n = int(nout.cpu()[0])
    ok, od = _oracle(oracle, cfg, img, 0)
    k = np.frombuffer(kps.cpu().numpy()[:n].tobytes(), dtype=ok.dtype)
    _same("odd pitch and base", (k, desc.cpu().numpy()[:n]), (ok, od))
    assert n >= 200


def test_forms_agree(pkg, oracle, monkeypatch):
    W, H = 320, 240
    cfg = (500, 1.2, 4, 20, 7)
    imgs = [synth.image(40 + i, W, H) for i in range(9)]
    ex_m = pkg.ORBextractor(*cfg, device=0, max_size=(W, H), max_batch=9)
    monkeypatch.setenv("ORBX_DESC_VALU_ROWPASS", "1")
    ex_v = pkg.ORBextractor(*cfg, device=0, max_size=(W, H), max_batch=9)
    monkeypatch.delenv("ORBX_DESC_VALU_ROWPASS")
    one_m, one_v = ex_m(imgs[0]), ex_v(imgs[0])
    assert ex_m.debug_launch_forms()["desc_rowpass"] == 2 and ex_v.debug_launch_forms()["desc_rowpass"] == 1
    want = _oracle(oracle, cfg, imgs[0], 0)
    _same("one image, matrix cores", one_m, want)
    _same("one image, vector ALUs", one_v, want)
    bm, bv = ex_m.extract_batch(imgs), ex_v.extract_batch(imgs)
    assert ex_m.debug_launch_forms()["desc_rowpass"] == 2 and ex_v.debug_launch_forms()["desc_rowpass"] == 1
    for i in range(9):
        assert len(bm[i][0]) >= 200
        assert bm[i][0].tobytes() == bv[i][0].tobytes() and bm[i][1].tobytes() == bv[i][1].tobytes(), f"image {i} of the batch: the forms differ"
    _same("image 0 of the batch", bm[0], want)
    _same("image 8 of the batch", bm[8], _oracle(oracle, cfg, imgs[8], 0))
