"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle on the same seeded
inputs.  Bar: bit-exact (integer / byte / index work; the fp32 fields of cv::KeyPoint are compared
by bit pattern as well)."""
import numpy as np
import pytest

from tools import synth

pytestmark = pytest.mark.gpu

ORB = dict(scaleFactor=1.2, nlevels=8, iniThFAST=20, minThFAST=7)


def _extractor(pkg, nfeatures, w, h, nlevels=8, max_batch=1):
    return pkg.ORBextractor(nfeatures, 1.2, nlevels, 20, 7, device=0, max_size=(w, h), max_batch=max_batch)


def _check_stages(ex, orc, img, tag):
    """compare stage by stage so that a failure names the first stage that diverges"""
    kps, desc = ex(img)
    okps, odesc = orc.extract(img)
    for l in range(orc.nlevels):
        g = ex.pyramid_level(l)
        o = orc.level(l)
        assert g.shape == o.shape, f"{tag}: level {l} shape {g.shape} vs {o.shape}"
        bad = np.argwhere(g != o)
        assert len(bad) == 0, f"{tag}: pyramid level {l}: {len(bad)} pixels differ, first at {bad[:3].tolist()}"
    for l in range(orc.nlevels):
        gx, gy, gr = ex.debug_candidates(l)
        ox, oy, orr = orc.candidates(l)
        assert len(gx) == len(ox), f"{tag}: level {l}: {len(gx)} FAST candidates vs oracle {len(ox)}"
        assert (gx == ox).all() and (gy == oy).all(), f"{tag}: level {l}: candidate positions/order differ"
        assert (gr == orr).all(), f"{tag}: level {l}: candidate responses differ"
    gc = ex.debug_level_counts()
    oc = np.array([orc.nkeypoints(l) for l in range(orc.nlevels)])
    assert (gc == oc).all(), f"{tag}: keypoints per level {gc.tolist()} vs oracle {oc.tolist()}"
    assert len(kps) == len(okps)
    for f in ("x", "y", "octave", "response", "size", "class_id"):
        bad = np.nonzero(kps[f] != okps[f])[0]
        assert len(bad) == 0, f"{tag}: keypoint field {f} differs at {bad[:5].tolist()} (quadtree selection/order)"
    bad = np.nonzero(kps["angle"].view(np.uint32) != okps["angle"].view(np.uint32))[0]
    assert len(bad) == 0, f"{tag}: angle bits differ at {bad[:5].tolist()}: {kps['angle'][bad[:3]]} vs {okps['angle'][bad[:3]]}"
    bad = np.nonzero((desc != odesc).any(axis=1))[0]
    assert len(bad) == 0, f"{tag}: {len(bad)} descriptors differ, first {bad[:5].tolist()}"
    assert kps.tobytes() == okps.tobytes()
    return kps, desc


def test_cv_profile_3_4_2(pkg, oracle):
    """the GaussianBlur taps of OpenCV >= 3.4.2 (orbx_extractor_set_cv_profile): same keypoints, other descriptors, and still the
    oracle's byte for byte; switching back restores the 3.2 descriptors"""
    img = synth.image(6, 640, 480)
    ex = _extractor(pkg, 1000, 640, 480)
    orc = oracle.Oracle(1000, 1.2, 8, 20, 7)
    k0, d0 = _check_stages(ex, orc, img, "profile 3.2")
    ex.set_cv_profile(pkg.orbx.CV_PROFILE_3_4_2); orc.set_cv_profile(1)
    k1, d1 = _check_stages(ex, orc, img, "profile 3.4.2")
    assert k0.tobytes() == k1.tobytes() and (d0 != d1).any(axis=1).sum() > 100
    ex.set_cv_profile(pkg.orbx.CV_PROFILE_3_2); orc.set_cv_profile(0)
    k2, d2 = _check_stages(ex, orc, img, "profile 3.2 again")
    assert d2.tobytes() == d0.tobytes()
    with pytest.raises(pkg.OrbxError):
        ex.set_cv_profile(7)


@pytest.mark.parametrize("w,h,nf,seed", [(320, 240, 500, 1), (640, 480, 1000, 2), (752, 480, 1000, 3), (1241, 376, 2000, 4)])
def test_extract_stage_parity(pkg, oracle, w, h, nf, seed):
    img = synth.image(seed, w, h)
    ex = _extractor(pkg, nf, w, h)
    orc = oracle.Oracle(nf, 1.2, 8, 20, 7)
    _check_stages(ex, orc, img, f"{w}x{h}")


@pytest.mark.parametrize("groups", ["2,5", "7", "1", "3,4", "1,2,4"])
def test_pyramid_launch_forms(pkg, oracle, monkeypatch, groups):
    """ComputePyramid (src/ORBextractor.cc:1347-1370) has two launch forms: one launch per level (batches) and several levels per launch
    (k_pyr_group, small launches).  Every grouping and the per-level form give the oracle's pyramid and keypoints bit for bit, on sizes
    whose tiles end in partial columns / rows, for other scale factors, and for a level-0 image at an odd address and pitch."""
    monkeypatch.setenv("ORBX_PYR_GROUPS", groups)
    for (w, h, nf, sf, nl) in [(1241, 376, 1000, 1.2, 8), (640, 480, 800, 1.2, 8), (333, 257, 300, 1.2, 6), (752, 480, 700, 1.5, 4),
                               (517, 389, 500, 1.1, 8), (1000, 700, 900, 1.9, 3), (1920, 1080, 2000, 1.2, 8)]:
        img = synth.image(w + h, w, h, nshapes=int(w * h / 400) + 50)
        orc = oracle.Oracle(nf, sf, nl, 20, 7)
        ex = pkg.ORBextractor(nf, sf, nl, 20, 7, device=0, max_size=(w, h))
        ex.set_pyramid_group_limit(0)
        k0, d0 = _check_stages(ex, orc, img, f"{w}x{h} sf {sf} per-level launches")
        ex.set_pyramid_group_limit(64)
        k1, d1 = _check_stages(ex, orc, img, f"{w}x{h} sf {sf} groups {groups}")
        assert k0.tobytes() == k1.tobytes() and d0.tobytes() == d1.tobytes()
    # mid-sized launches: the first group's levels by one launch each, the later groups grouped (limit 0 < 1 image <= the mid limit)
    monkeypatch.setenv("ORBX_PYR_GROUP_MID_IMAGES", "64")
    monkeypatch.setenv("ORBX_PYR_GROUP_MAX_IMAGES", "0")
    ex = pkg.ORBextractor(nf, sf, nl, 20, 7, device=0, max_size=(w, h))
    k2, d2 = _check_stages(ex, orc, img, f"{w}x{h} sf {sf} groups {groups}, mid regime")
    assert k0.tobytes() == k2.tobytes() and d0.tobytes() == d2.tobytes()
    with pytest.raises(pkg.OrbxError):
        ex.set_pyramid_group_limit(-1)


@pytest.mark.parametrize("nw", ["1", "2", "3", "4"])
def test_fast_waves_per_cell(pkg, oracle, monkeypatch, nw):
    """k_fast runs a cell on one wave (batches) or on several (a frame or two: the launch lasts as long as its fullest cell): every
    split gives the oracle's candidates, in order, incl. cells fuller than the candidate list (rounds) and the minThFAST fallback"""
    monkeypatch.setenv("ORBX_FAST_WAVES", nw)
    for (w, h, nf, kind) in [(1241, 376, 1000, "scene"), (640, 480, 800, "checker"), (333, 257, 300, "scene"), (640, 480, 500, "lowcontrast")]:
        if kind == "scene":
            img = synth.image(w + int(nw), w, h, nshapes=int(w * h / 300) + 50)
        elif kind == "checker":          # dense corners: candidate lists beyond ORBX_FAST_LIST_CAP
            yy, xx = np.mgrid[0:h, 0:w]
            img = (((xx // 3 + yy // 3) & 1) * 200 + 20).astype(np.uint8)
        else:                            # contrast between minThFAST and iniThFAST: every cell takes the second pass
            rng = np.random.Generator(np.random.PCG64(5))
            img = (100 + (synth.image(9, w, h).astype(np.int32) - 100) // 14).astype(np.uint8)
        orc = oracle.Oracle(nf, 1.2, 8, 20, 7)
        ex = pkg.ORBextractor(nf, 1.2, 8, 20, 7, device=0, max_size=(w, h))
        _check_stages(ex, orc, img, f"{w}x{h} {kind} fast waves {nw}")


@pytest.mark.parametrize("pair", ["0", "1"])
def test_fast_pair_kernel(pkg, oracle, monkeypatch, pair):
    """k_fast2 (batches: one wave per PAIR of horizontally adjacent FAST cells, shared halo, one concatenated candidate list) against
    k_fast (one cell per wave) on the same inputs, both against the oracle stage by stage: per-cell non-maximum suppression across the
    A | B boundary, the per-cell minThFAST fallback (only the cell that kept nothing runs again), odd column counts (a cell alone),
    narrow / skipped last columns, detect areas taller than 32 rows (whole-row bitmap segments), candidate lists beyond the cap
    (rounds), and shapes whose cells are wider than 32 px (the pair kernel must step aside)"""
    monkeypatch.setenv("ORBX_FAST_PAIR", pair)
    monkeypatch.setenv("ORBX_FAST_WAVES", "1")
    rng = np.random.Generator(np.random.PCG64(17))
    cases = [(1241, 376, 1000, "scene"), (640, 480, 800, "checker"), (333, 257, 300, "scene"), (640, 480, 500, "lowcontrast"),
             (752, 480, 1000, "halfflat"), (1920, 1080, 2000, "scene"), (783, 814, 1500, "scene"), (401, 299, 400, "noise"), (262, 226, 200, "scene")]
    for (w, h, nf, kind) in cases:
        if kind == "scene":
            img = synth.image(w + 3, w, h, nshapes=int(w * h / 300) + 50)
        elif kind == "checker":          # dense corners: candidate lists beyond ORBX_FAST_LIST_CAP
            yy, xx = np.mgrid[0:h, 0:w]
            img = (((xx // 3 + yy // 3) & 1) * 200 + 20).astype(np.uint8)
        elif kind == "noise":
            img = rng.integers(0, 256, (h, w), dtype=np.uint8)
        elif kind == "halfflat":         # columns alternate between textured and low-contrast 31-px stripes: in most pairs exactly ONE cell falls back to minThFAST
            img = synth.image(23, w, h, nshapes=1500)
            low = (100 + (img.astype(np.int32) - 100) // 14).astype(np.uint8)
            stripe = ((np.arange(w) - 16) // 31) % 2 == 1
            img = np.where(stripe[None, :], low, img).astype(np.uint8)
        else:                            # contrast between minThFAST and iniThFAST: every cell takes the second pass
            img = (100 + (synth.image(9, w, h).astype(np.int32) - 100) // 14).astype(np.uint8)
        orc = oracle.Oracle(nf, 1.2, 8, 20, 7)
        ex = pkg.ORBextractor(nf, 1.2, 8, 20, 7, device=0, max_size=(w, h))
        _check_stages(ex, orc, img, f"{w}x{h} {kind} pair kernel {pair}")
        # the form really ran (k_fast2 needs every cell at most 32 px wide: 640x480 has 33-px cells at levels 2 and 5)
        # the form really ran: k_fast2 needs every cell at most 32 px wide (640x480 and 752x480 have a level of 33-px cells)
        pair_ok = all(-(-(lw - 32) // ((lw - 32) // 30)) <= 32 for lw in [int(np.rint(np.float32(w) / s_)) for s_ in np.cumprod([1.0] + [np.float32(1.2)] * 7, dtype=np.float32)])
        assert ex.debug_fast_form() == (2 if pair == "1" and pair_ok else 1), (w, h, ex.debug_fast_form())
    for sf, nl in ((1.5, 4), (1.1, 6)):
        img = synth.image(7, 640, 480)
        _check_stages(pkg.ORBextractor(800, sf, nl, 20, 7, device=0, max_size=(640, 480)), oracle.Oracle(800, sf, nl, 20, 7), img, f"sf={sf} pair kernel {pair}")


def test_extract_fhd_4000(pkg, oracle):
    img = synth.image(5, 1920, 1080, nshapes=4000)
    ex = _extractor(pkg, 4000, 1920, 1080)
    orc = oracle.Oracle(4000, 1.2, 8, 20, 7)
    assert (ex.GetFeaturesPerLevel() == orc.features_per_level()).all()
    _check_stages(ex, orc, img, "fhd")


def test_one_pixel_wide_cells(pkg, oracle):
    """783 / 814 give a last FAST cell that is exactly 7 px wide / high: one detectable column / row"""
    img = synth.image(6, 783, 814, nshapes=2500)
    ex = _extractor(pkg, 1500, 783, 814)
    orc = oracle.Oracle(1500, 1.2, 8, 20, 7)
    _check_stages(ex, orc, img, "783x814")


@pytest.mark.parametrize("sf,nlevels", [(1.5, 4), (1.1, 6), (1.9, 3), (2.0, 3), (1.1, 16), (1.2, 12)])
def test_other_scale_factors(pkg, oracle, sf, nlevels):
    """non-default scaleFactor: resize tables, quotas and (for large factors) the non-LDS resize path"""
    img = synth.image(7, 640, 480)
    ex = pkg.ORBextractor(800, sf, nlevels, 20, 7, device=0, max_size=(640, 480))
    orc = oracle.Oracle(800, sf, nlevels, 20, 7)
    _check_stages(ex, orc, img, f"sf={sf}")


def test_random_geometry_sweep(pkg, oracle):
    """seeded sweep over image sizes / feature counts / level counts / scale factors: every combination changes the
    cell grid, the resize tables, the quadtree roots and the LDS carve; all stages must stay bit-exact"""
    rng = np.random.Generator(np.random.PCG64(2024))
    done = big = 0
    for trial in range(60):
        w = int(rng.integers(120, 1400)); h = int(rng.integers(100, 900))
        nlevels = int(rng.integers(1, 9)); sf = float(rng.choice([1.1, 1.2, 1.2, 1.2, 1.25, 1.4, 1.7]))
        nf = int(rng.integers(50, 3000)) if trial % 6 else int(rng.integers(9000, 16000))   # every sixth: beyond the LDS node tables
        try:
            orc = oracle.Oracle(nf, sf, nlevels, 20, 7)
            img = synth.image(3000 + trial, w, h, nshapes=int(w * h / 400) + 50)
            okps, odesc = orc.extract(img)
        except RuntimeError:
            # the oracle rejects what the reference cannot process (top level smaller than a cell, zero roots)
            ex = pkg.ORBextractor(nf, sf, nlevels, 20, 7, device=0, max_size=(w, h))
            with pytest.raises(pkg.OrbxError):
                ex(np.zeros((h, w), np.uint8))
            continue
        ex = pkg.ORBextractor(nf, sf, nlevels, 20, 7, device=0, max_size=(w, h))
        tag = f"trial {trial}: {w}x{h} nf={nf} levels={nlevels} sf={sf}"
        big += int(orc.features_per_level().max() > 2050)   # node tables in the HBM workspace instead of LDS (same code path otherwise)
        kps, desc = ex(img)
        assert len(kps) == len(okps), tag
        assert kps.tobytes() == okps.tobytes(), tag
        assert desc.tobytes() == odesc.tobytes(), tag
        done += 1
    assert done >= 40 and big >= 3


def test_large_nfeatures_hbm_node_tables(pkg, oracle):
    """nfeatures far beyond ORB-SLAM2's settings (src/ORBextractor.cc:468-493 accepts any): per-level quotas of several
    thousand leaves put the quadtree's node tables into the HBM workspace; same results as the oracle.  The only remaining bound is
    the 14-bit node id of the point labels (about 16 000 leaves per level)."""
    w, h = 1241, 376
    img = synth.image(77, w, h, nshapes=4000)
    for nf in (12000, 24000):
        ex = pkg.ORBextractor(nf, 1.2, 8, 20, 7, device=0, max_size=(w, h))
        orc = oracle.Oracle(nf, 1.2, 8, 20, 7)
        assert orc.features_per_level().max() > 2500
        kps, desc = ex(img)
        okps, odesc = orc.extract(img)
        assert len(kps) == len(okps) > 6000 and kps.tobytes() == okps.tobytes() and desc.tobytes() == odesc.tobytes(), nf
    with pytest.raises(pkg.OrbxError, match="quadtree labels hold"):
        pkg.ORBextractor(120000, 1.2, 8, 20, 7, device=0, max_size=(w, h))(img)


def test_two_handles_two_threads(pkg, oracle):
    """distinct handles may be used concurrently from different host threads"""
    import threading
    imgs = [synth.image(90 + i, 640, 480) for i in range(2)]
    exp = [oracle.Oracle(1000, 1.2, 8, 20, 7).extract(im) for im in imgs]
    exs = [_extractor(pkg, 1000, 640, 480) for _ in range(2)]
    errs = []

    def work(i):
        try:
            for _ in range(20):
                k, d = exs[i](imgs[i])
                assert k.tobytes() == exp[i][0].tobytes() and d.tobytes() == exp[i][1].tobytes()
        except Exception as e:  # noqa: BLE001
            errs.append(e)
    ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    [t.start() for t in ts]; [t.join() for t in ts]
    assert not errs, errs


def test_tables_match_oracle(pkg, oracle):
    ex = _extractor(pkg, 2000, 640, 480)
    orc = oracle.Oracle(2000, 1.2, 8, 20, 7)
    assert ex.GetLevels() == 8
    assert ex.GetScaleFactors().tobytes() == orc.scale_factors().tobytes()
    assert ex.GetInverseScaleFactors().tobytes() == orc.inv_scale_factors().tobytes()
    assert ex.GetScaleSigmaSquares().tobytes() == orc.level_sigma2().tobytes()
    assert ex.GetInverseScaleSigmaSquares().tobytes() == orc.inv_level_sigma2().tobytes()
    assert (ex.GetFeaturesPerLevel() == orc.features_per_level()).all()


@pytest.mark.parametrize("kind", ["flat", "low_contrast", "noise", "checker", "checker1", "dense_corners"])
def test_extract_edge_images(pkg, oracle, kind):
    """empty-ish / degenerate inputs: no corners, minThFAST fallback everywhere, saturated corner density.  "checker1" (every
    pixel passes k_fast's pretest, none is a corner) and "dense_corners" (binary noise: more than half of a cell's pixels are
    pretest candidates) overflow k_fast's candidate list (ORBX_FAST_LIST_CAP) and take the multi-round path"""
    w, h = 400, 300
    rng = np.random.default_rng(7)
    if kind == "flat":
        img = np.full((h, w), 128, np.uint8)
    elif kind == "low_contrast":
        img = (synth.image(9, w, h).astype(np.float32) * 0.12 + 100).astype(np.uint8)
    elif kind == "noise":
        img = rng.integers(0, 256, (h, w), dtype=np.uint8)
    elif kind == "checker":
        yy, xx = np.mgrid[0:h, 0:w]
        img = (((xx // 6 + yy // 6) & 1) * 200 + 20).astype(np.uint8)
    elif kind == "checker1":
        yy, xx = np.mgrid[0:h, 0:w]
        img = (((xx + yy) & 1) * 255).astype(np.uint8)
    else:
        img = rng.integers(0, 2, (h, w), dtype=np.uint8) * 255
    ex = _extractor(pkg, 800, w, h)
    orc = oracle.Oracle(800, 1.2, 8, 20, 7)
    kps, desc = _check_stages(ex, orc, img, kind)
    if kind == "flat":
        assert len(kps) == 0


def test_extract_empty_and_errors(pkg):
    ex = _extractor(pkg, 500, 640, 480)
    kps, desc = ex(np.zeros((0, 0), np.uint8))
    assert len(kps) == 0 and desc.shape == (0, 32)
    with pytest.raises(pkg.OrbxError):      # level 7 smaller than one FAST cell: reference divides by zero
        ex(np.zeros((120, 160), np.uint8))
    with pytest.raises(pkg.OrbxError):      # larger than the workspace
        ex(np.zeros((600, 800), np.uint8))
    with pytest.raises(pkg.OrbxError):      # not CV_8UC1
        ex(np.zeros((480, 640), np.float32))


def test_small_image_fewer_levels(pkg, oracle):
    img = synth.image(21, 160, 120, nshapes=300)
    ex = _extractor(pkg, 300, 160, 120, nlevels=4)
    orc = oracle.Oracle(300, 1.2, 4, 20, 7)
    _check_stages(ex, orc, img, "160x120/4 levels")


@pytest.mark.parametrize("ch,rgb", [(3, True), (3, False), (4, True), (4, False)])
def test_color_ingest(pkg, oracle, ch, rgb):
    """Tracking::GrabImage* colour path: cvtColor on device, then the extractor"""
    rng = np.random.default_rng(5)
    base = synth.image(33, 640, 480).astype(np.int32)
    col = np.stack([np.clip(base + rng.integers(-40, 40, base.shape), 0, 255) for _ in range(ch)], axis=2).astype(np.uint8)
    ex = _extractor(pkg, 1000, 640, 480)
    kps, desc, gray = ex.extract_color(col, rgb=rgb, want_gray=True)
    ogray = oracle.cvt_gray(col, rgb)
    assert (gray == ogray).all()
    okps, odesc = oracle.Oracle(1000, 1.2, 8, 20, 7).extract(ogray)
    assert kps.tobytes() == okps.tobytes() and desc.tobytes() == odesc.tobytes()
    # the weights are the usual luma weights: a pure-channel image lands on round(255 * w)
    pure = np.zeros((64, 64, ch), np.uint8); pure[..., 0] = 255
    assert oracle.cvt_gray(pure, True)[0, 0] == 76 and oracle.cvt_gray(pure, False)[0, 0] == 29


def test_strided_input(pkg, oracle):
    big = synth.image(31, 800, 500)
    view = big[10:490, 40:680]          # 640x480 view with row stride 800
    ex = _extractor(pkg, 1000, 640, 480)
    kps, desc = ex(view)
    okps, odesc = oracle.Oracle(1000, 1.2, 8, 20, 7).extract(np.ascontiguousarray(view))
    assert kps.tobytes() == okps.tobytes() and desc.tobytes() == odesc.tobytes()


def test_batch_equals_single(pkg, oracle):
    seq = synth.sequence(41, 640, 480, 6)
    ex = _extractor(pkg, 1000, 640, 480, max_batch=8)
    res = ex.extract_batch(list(seq))
    orc = oracle.Oracle(1000, 1.2, 8, 20, 7)
    for i, (k, d) in enumerate(res):
        ok, od = orc.extract(seq[i])
        assert k.tobytes() == ok.tobytes(), f"frame {i}"
        assert d.tobytes() == od.tobytes(), f"frame {i}"
    # the same handle, reused for a different size and back (geometry cache)
    k2, d2 = ex(synth.image(42, 320, 240))
    ok2, od2 = oracle.Oracle(1000, 1.2, 8, 20, 7).extract(synth.image(42, 320, 240))
    assert k2.tobytes() == ok2.tobytes() and d2.tobytes() == od2.tobytes()


def test_idempotent_and_deterministic(pkg):
    img = synth.image(51, 752, 480)
    ex = _extractor(pkg, 1000, 752, 480)
    a = ex(img); b = ex(img)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


# ------------------------------------------------------------------------------- stereo

def _stereo_case(pkg, oracle, seed, w, h, nf, sf=1.2, nlevels=8):
    left, right, disp = synth.stereo_pair(seed, w, h)
    exL = pkg.ORBextractor(nf, sf, nlevels, 20, 7, device=0, max_size=(w, h))
    exR = pkg.ORBextractor(nf, sf, nlevels, 20, 7, device=0, max_size=(w, h))
    kL, dL = exL(left); kR, dR = exR(right)
    oL, oR = oracle.Oracle(nf, sf, nlevels, 20, 7), oracle.Oracle(nf, sf, nlevels, 20, 7)
    okL, odL = oL.extract(left); okR, odR = oR.extract(right)
    assert kL.tobytes() == okL.tobytes() and kR.tobytes() == okR.tobytes()
    bf, b = 386.1448, 386.1448 / 718.856  # Examples/Stereo/KITTI00-02.yaml:8,25
    ur, dp = pkg.ComputeStereoMatches(exL, exR, kL, dL, kR, dR, bf, b)
    our, odp = oracle.stereo_match(oL, oR, okL, odL, okR, odR, bf, b)
    return ur, dp, our, odp, kL, disp


@pytest.mark.parametrize("seed,w,h,nf,sf,nlevels", [pytest.param(61, 640, 480, 1000, 1.2, 8, id="61-640-480-1000"),
                                                   pytest.param(62, 1241, 376, 2000, 1.2, 8, id="62-1241-376-2000"),
                                                   (65, 1241, 376, 2000, 1.1, 16), (66, 752, 480, 1000, 1.9, 4)])
def test_stereo_parity(pkg, oracle, seed, w, h, nf, sf, nlevels):
    """other scale factors change the per-level row reach of the band search (orbx_stereo.hip: tabs.reach_pk)"""
    ur, dp, our, odp, kL, disp = _stereo_case(pkg, oracle, seed, w, h, nf, sf, nlevels)
    bad = np.nonzero(ur.view(np.uint32) != our.view(np.uint32))[0]
    assert len(bad) == 0, f"uRight differs at {bad[:5].tolist()}: {ur[bad[:5]]} vs {our[bad[:5]]}"
    assert dp.tobytes() == odp.tobytes()
    assert (ur >= 0).sum() > 50  # the test is not vacuous
    # size-independent property: recovered disparities agree with the generator's disparity field
    ok = ur >= 0
    d_true = disp[np.clip(kL["y"].astype(int), 0, len(disp) - 1)]
    assert (np.abs((kL["x"] - ur)[ok] - d_true[ok]) < 2.0).mean() > 0.8


@pytest.mark.parametrize("kpw,rowtab", [("1", True), ("4", True), ("1", False), ("4", False)])
def test_stereo_launch_forms(pkg, oracle, monkeypatch, kpw, rowtab):
    """ComputeStereoMatches has two wave shapes (one / four left keypoints per wave: single frames / batches) and two sources of the
    row table (built inside the descriptor launch of the right image, or by k_stereo_prep for keypoints handed in by the caller):
    all four combinations give the oracle's uRight / depth bit for bit, through the host API and through the single-call form"""
    monkeypatch.setenv("ORBX_STEREO_KPW", kpw)
    if not rowtab:
        monkeypatch.setenv("ORBX_NO_ROWTAB", "1")
    for seed, w, h, nf in [(63, 1241, 376, 1000), (64, 640, 480, 1200)]:
        ur, dp, our, odp, kL, disp = _stereo_case(pkg, oracle, seed, w, h, nf)
        assert ur.tobytes() == our.tobytes() and dp.tobytes() == odp.tobytes() and (ur >= 0).sum() > 50
        left, right, _ = synth.stereo_pair(seed, w, h)
        ex = pkg.ORBextractor(nf, 1.2, 8, 20, 7, device=0, max_size=(w, h), max_batch=2)
        r = ex.extract_stereo(left, right, 386.1448, 386.1448 / 718.856)
        assert r[4].tobytes() == our.tobytes() and r[5].tobytes() == odp.tobytes()


def test_stereo_row_table_sources_device(pkg, oracle):
    """where orbx_stereo_match_batch_device takes its row table from is an ARGUMENT (never inferred from addresses): ROWTAB_OF_EXTRACTION
    = the by-product of the right image's extraction (refused when the buffer / capacity / image range cannot be that extraction's),
    ROWTAB_FROM_KEYPOINTS = built from whatever keypoints are handed in -- also the extraction's own buffer EDITED IN PLACE, the case
    the pointer-identity rule of round 3 got silently wrong"""
    import torch
    w, h, nf = 1241, 376, 1000
    bf, b = 386.1448, 386.1448 / 718.856
    left, right, _ = synth.stereo_pair(91, w, h)
    pitch = (w + 63) // 64 * 64
    host = np.zeros((2, h, pitch), np.uint8); host[0, :, :w] = left; host[1, :, :w] = right
    imgs = torch.from_numpy(host).cuda()
    ex = pkg.ORBextractor(nf, 1.2, 8, 20, 7, device=0, max_size=(w, h), max_batch=2)
    cap = ex.max_keypoints(w, h)
    kps = torch.zeros((2, cap, 7), device="cuda"); desc = torch.zeros((2, cap, 32), dtype=torch.uint8, device="cuda")
    n = torch.zeros(2, dtype=torch.int32, device="cuda")
    ur = torch.zeros(cap, device="cuda"); dp = torch.zeros(cap, device="cuda")
    ex.extract_batch_device(imgs.data_ptr(), h * pitch, pitch, 2, w, h, kps.data_ptr(), desc.data_ptr(), cap, n.data_ptr(), None)
    oL, oR = oracle.Oracle(nf, 1.2, 8, 20, 7), oracle.Oracle(nf, 1.2, 8, 20, 7)
    okL, odL = oL.extract(left); okR, odR = oR.extract(right)
    X, K = pkg.orbx.ROWTAB_OF_EXTRACTION, pkg.orbx.ROWTAB_FROM_KEYPOINTS

    def run(kr_ptr, src):
        pkg.orbx.stereo_match_batch_device(ex, 0, ex, 1, 1, kps.data_ptr(), desc.data_ptr(), n.data_ptr(), kr_ptr, desc[1:].data_ptr(), n[1:].data_ptr(),
                                           cap, bf, b, ur.data_ptr(), dp.data_ptr(), None, row_table=src)
        ex.sync()
        nl = int(n[0].item())
        return ur.cpu().numpy()[:nl].copy(), dp.cpu().numpy()[:nl].copy()
    our, odp = oracle.stereo_match(oL, oR, okL, odL, okR, odR, bf, b)
    assert pkg.orbx.stereo_row_table_available(ex, kps[1:].data_ptr(), 1, 1, cap)
    for src in (X, K):                                           # the extraction's own buffer: by-product table, or one built from it
        g_ur, g_dp = run(kps[1:].data_ptr(), src)
        assert g_ur.tobytes() == our.tobytes() and g_dp.tobytes() == odp.tobytes() and (our >= 0).sum() > 50
    clone = kps[1:].clone()                                      # the same keypoints at another address: k_stereo_prep
    g_ur, g_dp = run(clone.data_ptr(), K)
    assert g_ur.tobytes() == our.tobytes() and g_dp.tobytes() == odp.tobytes()
    assert not pkg.orbx.stereo_row_table_available(ex, clone.data_ptr(), 1, 1, cap)
    with pytest.raises(pkg.OrbxError):                           # a buffer that cannot be the extraction's: the claim is refused, not believed
        run(clone.data_ptr(), X)
    with pytest.raises(pkg.OrbxError):
        run(kps[1:].data_ptr(), 7)
    ed = okR.copy()                                              # an edited copy: a third of the right keypoints moved 40 rows down
    ed["y"][::3] += 40.0
    edited = torch.from_numpy(np.pad(ed.view(np.uint8).reshape(len(ed), 28), ((0, cap - len(ed)), (0, 0))).copy()).cuda()
    eur, edp = oracle.stereo_match(oL, oR, okL, odL, ed, odR, bf, b)
    g_ur, g_dp = run(edited.data_ptr(), K)
    assert g_ur.tobytes() == eur.tobytes() and g_dp.tobytes() == edp.tobytes() and eur.tobytes() != our.tobytes()
    kps[1].view(torch.uint8).view(-1)[:edited.numel()] = edited.view(-1)     # ... and the extraction's own buffer edited IN PLACE
    g_ur, g_dp = run(kps[1:].data_ptr(), K)
    assert g_ur.tobytes() == eur.tobytes() and g_dp.tobytes() == edp.tobytes()


def test_stereo_rejects_bad_octave(pkg):
    w, h = 640, 480
    exL, exR = _extractor(pkg, 300, w, h), _extractor(pkg, 300, w, h)
    img = synth.image(72, w, h)
    kL, dL = exL(img); kR, dR = exR(img)
    bad = kR.copy(); bad["octave"][0] = 99
    with pytest.raises(pkg.OrbxError):
        pkg.ComputeStereoMatches(exL, exR, kL, dL, bad, dR, 386.1448, 0.5372)
    # identical eyes: every SAD is 0, so the median cut (thDist = 1.5*1.4*0) drops every match, as in the reference
    ur, dp = pkg.ComputeStereoMatches(exL, exR, kL, dL, kR, dR, 386.1448, 0.5372)
    assert (ur == -1).all() and (dp == -1).all()


def test_stereo_no_matches(pkg, oracle):
    """right eye unrelated to the left: (almost) nothing survives; empty accepted set must not fault"""
    w, h = 640, 480
    exL, exR = _extractor(pkg, 500, w, h), _extractor(pkg, 500, w, h)
    left = synth.image(71, w, h); right = np.full((h, w), 90, np.uint8)
    right[200:240, 300:340] = 200
    kL, dL = exL(left); kR, dR = exR(right)
    oL, oR = oracle.Oracle(500, 1.2, 8, 20, 7), oracle.Oracle(500, 1.2, 8, 20, 7)
    okL, odL = oL.extract(left); okR, odR = oR.extract(right)
    ur, dp = pkg.ComputeStereoMatches(exL, exR, kL, dL, kR, dR, 386.1448, 0.5372)
    our, odp = oracle.stereo_match(oL, oR, okL, odL, okR, odR, 386.1448, 0.5372)
    assert ur.tobytes() == our.tobytes() and dp.tobytes() == odp.tobytes()


# ------------------------------------------------------------------------------- BoW matchers

def _bow_sets(pkg, oracle, seed, n_kf=3, flip=0.05, vocab_k=10):
    rng = np.random.Generator(np.random.PCG64(seed))
    img = synth.image(seed, 752, 480)
    ex = _extractor(pkg, 1000, 752, 480)
    k, d = ex(img)
    voc = synth.Vocab2(seed + 1, k=vocab_k); voc.seed_from(d, rng)

    def mk(desc, kp, flag):
        ids, off, feat = voc.feature_vector(desc)
        return dict(desc=desc, node_id=ids, node_off=off, feat=feat, flag=flag, angle=kp["angle"],
                    x=kp["x"], y=kp["y"], octave=kp["octave"], u_right=np.where(rng.random(len(kp)) < 0.3, 5.0, -1.0).astype(np.float32))
    frame = mk(d, k, np.zeros(len(d), np.uint8))
    kfs = []
    for i in range(n_kf):
        perm = rng.permutation(len(d))
        dk = synth.flip_bits(rng, d, flip)[perm]
        kk = k[perm].copy()
        kk["angle"] = (kk["angle"] + rng.normal(0, 4 + 20 * i, len(kk)).astype(np.float32)) % np.float32(360)
        kfs.append(mk(dk, kk, (rng.random(len(d)) < 0.6).astype(np.uint8)))
    return frame, kfs, ex


def test_search_by_bow_many_nodes(pkg, oracle):
    """a k = 30 vocabulary: several hundred distinct nodes per feature vector, so the table kernel walks several chunks of BOW_CHUNK (256)
    nodes per pair (ORB-SLAM2's level-4 nodes give <= 100); both kernel forms, both search flavours"""
    frame, kfs, _ = _bow_sets(pkg, oracle, 83, vocab_k=30)
    assert len(frame["node_id"]) > 260 and all(len(kf["node_id"]) > 260 for kf in kfs)
    m = pkg.ORBmatcher(0.75, True)
    for form in ("wave", "table"):
        pkg.orbx.debug_set_bow_form(form)
        try:
            for i, kf in enumerate(kfs):
                got, n = m.SearchByBoW(kf, frame)
                exp, en = oracle.search_by_bow_kf_f(kf, frame, 0.75, True)
                assert n == en and (got == exp).all(), f"form {form} kf {i}"
            b = dict(kfs[1]); b["kind"] = "keyframe"
            got, n = m.SearchByBoW(kfs[0], b)
            exp, en = oracle.search_by_bow_kf_kf(kfs[0], b, 0.75, True)
            assert n == en and (got == exp).all(), f"form {form} kf-kf"
        finally:
            pkg.orbx.debug_set_bow_form("auto")


@pytest.mark.parametrize("ratio,ori", [(0.7, True), (0.75, True), (0.9, False)])
def test_search_by_bow_kf_f(pkg, oracle, ratio, ori):
    frame, kfs, _ = _bow_sets(pkg, oracle, 81)
    m = pkg.ORBmatcher(ratio, ori)
    for i, kf in enumerate(kfs):
        got, n = m.SearchByBoW(kf, frame)
        exp, en = oracle.search_by_bow_kf_f(kf, frame, ratio, ori)
        assert n == en, f"kf {i}: nmatches {n} vs {en}"
        assert (got == exp).all(), f"kf {i}: {np.nonzero(got != exp)[0][:5].tolist()}"
        assert n > 20
    got, n = m.SearchByBoWBatch(kfs, frame)
    for i, kf in enumerate(kfs):
        exp, en = oracle.search_by_bow_kf_f(kf, frame, ratio, ori)
        assert n[i] == en and (got[i] == exp).all()


def test_bow_database(pkg, oracle):
    """device-resident keyframe set: same answers as one call per keyframe, for several query frames"""
    frame, kfs, _ = _bow_sets(pkg, oracle, 85, n_kf=7)
    db = pkg.BowDatabase(kfs)
    for q, ratio in ((frame, 0.75), (kfs[3], 0.7)):
        got, n = db.search(q, ratio, True)
        for i, kf in enumerate(kfs):
            exp, en = oracle.search_by_bow_kf_f(kf, q, ratio, True)
            assert n[i] == en and (got[i] == exp).all(), i


def test_search_by_bow_kf_kf(pkg, oracle):
    frame, kfs, _ = _bow_sets(pkg, oracle, 82)
    m = pkg.ORBmatcher(0.75, True)
    for a in range(len(kfs)):
        b = dict(kfs[(a + 1) % len(kfs)]); b["kind"] = "keyframe"
        got, n = m.SearchByBoW(kfs[a], b)
        exp, en = oracle.search_by_bow_kf_kf(kfs[a], b, 0.75, True)
        assert n == en and (got == exp).all()
        assert n > 10


@pytest.mark.parametrize("only_stereo,ori", [(False, False), (False, True), (True, False)])
def test_search_for_triangulation(pkg, oracle, only_stereo, ori):
    frame, kfs, ex = _bow_sets(pkg, oracle, 83, flip=0.03)
    a, b = kfs[0], dict(frame)
    a = dict(a); a["flag"] = (np.arange(len(a["desc"])) % 3 == 0).astype(np.uint8)   # "already has a MapPoint"
    b["flag"] = (np.arange(len(b["desc"])) % 5 == 0).astype(np.uint8)
    F12 = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32)   # pure x-translation: epipolar lines are rows
    F12 = F12 + np.float32(2e-7) * np.arange(9, dtype=np.float32).reshape(3, 3)
    sf, sg = ex.GetScaleFactors(), ex.GetScaleSigmaSquares()
    m = pkg.ORBmatcher(0.6, ori)
    got = m.SearchForTriangulation(a, b, F12, 300.0, 200.0, sf, sg, bOnlyStereo=only_stereo)
    exp = oracle.search_for_triangulation(a, b, F12, 300.0, 200.0, sf, sg, 0.6, ori, only_stereo)
    assert got.shape == exp.shape, f"{got.shape} vs {exp.shape}"
    assert (got == exp).all()
    if not only_stereo:
        assert len(got) > 10


def test_bow_edge_cases(pkg, oracle):
    """disjoint vocab nodes, empty feature vector, all-flags-off"""
    frame, kfs, _ = _bow_sets(pkg, oracle, 84, n_kf=1)
    kf = kfs[0]
    m = pkg.ORBmatcher(0.75, True)
    # no valid map points
    k0 = dict(kf); k0["flag"] = np.zeros(len(kf["desc"]), np.uint8)
    got, n = m.SearchByBoW(k0, frame)
    assert n == 0 and (got == -1).all()
    # disjoint node ids
    k1 = dict(kf); k1["node_id"] = kf["node_id"] + np.uint32(100000)
    got, n = m.SearchByBoW(k1, frame)
    exp, en = oracle.search_by_bow_kf_f(k1, frame, 0.75, True)
    assert n == en == 0 and (got == exp).all()
    # empty feature vector on one side
    k2 = dict(kf); k2["node_id"] = np.zeros(0, np.uint32); k2["node_off"] = np.zeros(1, np.int32); k2["feat"] = np.zeros(0, np.uint32)
    got, n = m.SearchByBoW(k2, frame)
    assert n == 0 and (got == -1).all()
    # malformed CSR is rejected, not trusted
    k3 = dict(kf); k3["feat"] = kf["feat"].copy(); k3["feat"][0] = 10 ** 6
    with pytest.raises(pkg.OrbxError):
        m.SearchByBoW(k3, frame)


def test_hamming_host(pkg, oracle):
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, (200, 32), dtype=np.uint8); b = rng.integers(0, 256, (200, 32), dtype=np.uint8)
    for i in range(200):
        assert pkg.ORBmatcher.DescriptorDistance(a[i], b[i]) == oracle.hamming(a[i], b[i]) == int(np.unpackbits(a[i] ^ b[i]).sum())


@pytest.mark.gpu
def test_bow_searches_table_form(pkg, oracle, monkeypatch):
    """the same SearchByBoW parity cases through the throughput form of the kernel (LDS distance table + row fixpoint),
    which a call only picks by itself from 4096 pairs up (orbx_bow.hip: bow_launch)"""
    pkg.orbx.debug_set_bow_form("table")
    try:
        test_search_by_bow_kf_f(pkg, oracle, 0.75, True)
        test_search_by_bow_kf_f(pkg, oracle, 0.9, False)
        test_bow_database(pkg, oracle)
        test_search_by_bow_kf_kf(pkg, oracle)
        test_bow_edge_cases(pkg, oracle)
    finally:
        pkg.orbx.debug_set_bow_form("auto")


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,off", [(1241, 376, 1), (640, 480, 3), (401, 301, 2)])
def test_extract_device_unaligned_pitch_and_base(pkg, oracle, w, h, off):
    """device-resident input with pitch == width (odd) and a base pointer that is not 4-byte aligned: the kernels fetch
    with unaligned dword loads, so this is the same code path as the aligned case"""
    import torch
    B = 2
    imgs = [synth.image(90 + i, w, h) for i in range(B)]
    flat = np.zeros(off + B * w * h + 8, np.uint8)
    for i in range(B):
        flat[off + i * w * h: off + (i + 1) * w * h] = imgs[i].reshape(-1)
    d = torch.from_numpy(flat).cuda()
    ex = pkg.ORBextractor(800, 1.2, 8, 20, 7, device=0, max_size=(w, h), max_batch=B)
    cap = ex.max_keypoints(w, h)
    kps = torch.zeros((B, cap, 7), device="cuda"); desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
    n = torch.zeros(B, dtype=torch.int32, device="cuda")
    ex.extract_batch_device(d.data_ptr() + off, w * h, w, B, w, h, kps.data_ptr(), desc.data_ptr(), cap, n.data_ptr(), None)
    ex.sync()
    nn = n.cpu().numpy(); kk = kps.cpu().numpy().view(np.uint8).reshape(B, cap, 28); dd = desc.cpu().numpy()
    orc = oracle.Oracle(800, 1.2, 8, 20, 7)
    for i in range(B):
        okps, odesc = orc.extract(imgs[i])
        assert nn[i] == len(okps) > 100
        assert kk[i, :nn[i]].tobytes() == okps.tobytes() and dd[i, :nn[i]].tobytes() == odesc.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("seed,w,h,nf", [(63, 1241, 376, 1000), (64, 752, 480, 1200)])
def test_extract_stereo_single_call(pkg, oracle, seed, w, h, nf):
    """orbx_extract_stereo = both eyes' operator() + ComputeStereoMatches of Frame::Frame (src/Frame.cc:82-97) in one call"""
    left, right, _ = synth.stereo_pair(seed, w, h)
    bf, b = 386.1448, 386.1448 / 718.856
    ex = pkg.ORBextractor(nf, 1.2, 8, 20, 7, device=0, max_size=(w, h), max_batch=2)
    kL, dL, kR, dR, ur, dp = ex.extract_stereo(left, right, bf, b)
    oL, oR = oracle.Oracle(nf, 1.2, 8, 20, 7), oracle.Oracle(nf, 1.2, 8, 20, 7)
    okL, odL = oL.extract(left); okR, odR = oR.extract(right)
    assert kL.tobytes() == okL.tobytes() and kR.tobytes() == okR.tobytes() and dL.tobytes() == odL.tobytes() and dR.tobytes() == odR.tobytes()
    our, odp = oracle.stereo_match(oL, oR, okL, odL, okR, odR, bf, b)
    assert ur.tobytes() == our.tobytes() and dp.tobytes() == odp.tobytes() and (ur >= 0).sum() > 50
    with pytest.raises(pkg.OrbxError):
        pkg.ORBextractor(nf, 1.2, 8, 20, 7, device=0, max_size=(w, h), max_batch=1).extract_stereo(left, right, bf, b)


@pytest.mark.gpu
def test_stereo_border_windows(pkg, oracle):
    """keypoints placed by hand right at the image border: their 11x11 SAD windows leave the level, so k_stereo takes
    the reflect-101 byte path instead of the dword/LDS path every extractor keypoint takes; same answers as the oracle"""
    w, h, nf = 752, 480, 800
    left, right, _ = synth.stereo_pair(66, w, h)
    exL, exR = _extractor(pkg, nf, w, h), _extractor(pkg, nf, w, h)
    kL, dL = exL(left); kR, dR = exR(right)
    oL, oR = oracle.Oracle(nf, 1.2, 8, 20, 7), oracle.Oracle(nf, 1.2, 8, 20, 7)
    oL.extract(left); oR.extract(right)          # the oracle's SAD stage reads its own pyramids
    rng = np.random.Generator(np.random.PCG64(67))
    m = 120
    kL2, dL2, kR2, dR2 = kL.copy(), dL.copy(), kR.copy(), dR.copy()
    idx = rng.choice(min(len(kL), len(kR)), m, replace=False)
    for t, i in enumerate(idx):
        lvl = int(rng.integers(0, 4)); s = np.float32(1.2) ** lvl
        lw, lh = int(round(w / float(s))), int(round(h / float(s)))
        edge = t % 4
        x = [rng.uniform(13, 17), rng.uniform(lw - 9, lw - 6.5), rng.uniform(40, lw - 40), rng.uniform(40, lw - 40)][edge]
        y = [rng.uniform(30, lh - 30), rng.uniform(30, lh - 30), rng.uniform(1, 5), rng.uniform(lh - 6, lh - 2)][edge]
        d = rng.uniform(0.5, 6.0)
        kL2["x"][i] = np.float32(x * s); kL2["y"][i] = np.float32(y * s); kL2["octave"][i] = lvl
        kR2["x"][i] = np.float32((x - d) * s); kR2["y"][i] = kL2["y"][i]; kR2["octave"][i] = lvl
        dR2[i] = dL2[i]                           # identical descriptors: the coarse stage pairs them
    bf, b = 386.1448, 386.1448 / 718.856
    ur, dp = pkg.ComputeStereoMatches(exL, exR, kL2, dL2, kR2, dR2, bf, b)
    our, odp = oracle.stereo_match(oL, oR, kL2, dL2, kR2, dR2, bf, b)
    assert ur.tobytes() == our.tobytes() and dp.tobytes() == odp.tobytes()
    assert (our[idx] >= 0).sum() >= 5 or (our >= 0).sum() > 50


@pytest.mark.gpu
@pytest.mark.parametrize("pinned,transport", [(False, {}), (True, {}), (True, {"ORBX_PIPE_KCOPY": "0"}), (False, {"ORBX_PIPE_KCOPY": "0"}),
                                              (True, {"ORBX_PIPE_INLINE": "0", "ORBX_PIPE_LANES": "2"}), (True, {"ORBX_PIPE_LANES": "1"}),
                                              (False, {"ORBX_PIPE_LANES": "3"})])
def test_extract_stereo_pipelined(pkg, oracle, monkeypatch, pinned, transport):
    """orbx_extract_stereo_submit / _wait: frames in flight up to the pipeline depth, results per ticket equal the oracle's
    (and the synchronous one-call form); resubmitting a slot before its wait is refused.  Every transport of the frames -- copy kernel on
    the frame's lane stream (default), copy engines on the lane stream, copy engines on two copy streams -- and 1 to 4 kernel lanes"""
    for k, v in transport.items():
        monkeypatch.setenv(k, v)
    w, h, nf = 1241, 376, 1000
    bf, b = 386.1448, 386.1448 / 718.856
    depth = pkg.orbx.pipeline_depth()
    nframes = 2 * depth + 1
    pairs = [synth.stereo_pair(700 + i, w, h)[:2] for i in range(3)]
    pairs[1] = (np.full((h, w), 50, np.uint8), np.full((h, w), 50, np.uint8))      # a featureless frame inside the stream
    exp = []
    for l, r in pairs:
        oL, oR = oracle.Oracle(nf, 1.2, 8, 20, 7), oracle.Oracle(nf, 1.2, 8, 20, 7)
        kL, dL = oL.extract(l); kR, dR = oR.extract(r)
        exp.append((kL, dL, kR, dR) + tuple(oracle.stereo_match(oL, oR, kL, dL, kR, dR, bf, b)))
    if pinned:
        bufs = []
        for l, r in pairs:
            pl, pr_ = pkg.orbx.pinned_array((h, w)), pkg.orbx.pinned_array((h, w))
            pl[:] = l; pr_[:] = r
            bufs.append((pl, pr_))
        pairs = bufs
    ex = pkg.ORBextractor(nf, 1.2, 8, 20, 7, device=0, max_size=(w, h), max_batch=2)
    tickets = []
    for i in range(depth):
        tickets.append(ex.extract_stereo_submit(pairs[i % 3][0], pairs[i % 3][1], bf, b))
    with pytest.raises(pkg.OrbxError):                       # every slot is in flight
        ex.extract_stereo_submit(pairs[0][0], pairs[0][1], bf, b)
    done = 0
    for i in range(depth, nframes + depth):
        t = tickets.pop(0)
        got = ex.extract_stereo_wait(t)
        e = exp[done % 3]
        for g_, e_ in zip(got, e):
            assert g_.tobytes() == e_.tobytes(), f"frame {done} (ticket {t})"
        done += 1
        if i < nframes:
            tickets.append(ex.extract_stereo_submit(pairs[i % 3][0], pairs[i % 3][1], bf, b))
    assert done == nframes and not tickets
    with pytest.raises(pkg.OrbxError):                       # a ticket can be waited for once
        ex.extract_stereo_wait(t)
    # the synchronous forms still work on the same handle afterwards
    got = ex.extract_stereo(np.asarray(pairs[2][0]), np.asarray(pairs[2][1]), bf, b)
    for g_, e_ in zip(got, exp[2]):
        assert g_.tobytes() == e_.tobytes()


@pytest.mark.gpu
def test_extract_pipelined_mono_and_mixed(pkg, oracle):
    """orbx_extract_submit / _wait (monocular stream), interleaved with stereo tickets on the same handle, and across a change
    of image size while frames are in flight"""
    bf, b = 386.1448, 386.1448 / 718.856
    ex = pkg.ORBextractor(800, 1.2, 8, 20, 7, device=0, max_size=(752, 480), max_batch=2)
    orc = oracle.Oracle(800, 1.2, 8, 20, 7)
    a = [synth.image(810 + i, 752, 480) for i in range(3)]
    small = synth.image(820, 640, 360)
    t0 = ex.extract_submit(a[0]); t1 = ex.extract_submit(a[1])
    l, r, _ = synth.stereo_pair(830, 752, 480)
    t2 = ex.extract_stereo_submit(l, r, bf, b)
    for t, im in ((t0, a[0]), (t1, a[1])):
        k, d = ex.extract_wait(t)
        ok, od = orc.extract(im)
        assert k.tobytes() == ok.tobytes() and d.tobytes() == od.tobytes()
    with pytest.raises(pkg.OrbxError):          # a stereo ticket cannot be collected through the mono form
        ex.extract_wait(t2)
    got = ex.extract_stereo_wait(t2)
    oL, oR = oracle.Oracle(800, 1.2, 8, 20, 7), oracle.Oracle(800, 1.2, 8, 20, 7)
    kL, dL = oL.extract(l); kR, dR = oR.extract(r)
    exp = (kL, dL, kR, dR) + tuple(oracle.stereo_match(oL, oR, kL, dL, kR, dR, bf, b))
    for g_, e_ in zip(got, exp):
        assert g_.tobytes() == e_.tobytes()
    # size change with a frame in flight: the new geometry waits for it, its results stay valid
    t3 = ex.extract_submit(a[2])
    t4 = ex.extract_submit(small)
    k, d = ex.extract_wait(t3); ok, od = orc.extract(a[2])
    assert k.tobytes() == ok.tobytes() and d.tobytes() == od.tobytes()
    k, d = ex.extract_wait(t4); ok, od = orc.extract(small)
    assert k.tobytes() == ok.tobytes() and d.tobytes() == od.tobytes()


def test_profile_stage_selection(pkg):
    """orbx_profile_enable / orbx_profile_stages: events are recorded for the selected stages only, one launch each per call
    (seven k_resize launches, or the two grouped pyramid launches of a small batch), and the outputs do not depend on profiling"""
    w, h = 640, 480
    img = synth.image(5, w, h)
    ex = _extractor(pkg, 800, w, h)
    k0, d0 = ex(img)
    ex.profile_read(reset=True)
    ex.profile_enable(True)
    k1, d1 = ex(img)
    ex.set_pyramid_group_limit(0)
    k2, d2 = ex(img)
    ex.profile_enable(False)
    prof = ex.profile_read(reset=True)
    assert k1.tobytes() == k0.tobytes() and (d1 == d0).all() and k2.tobytes() == k0.tobytes() and (d2 == d0).all()
    assert prof["resize"][1] == 2 + 7 and prof["fast"][1] == 2 and prof["tree"][1] == 2 and prof["desc"][1] == 2
    ex.profile_enable(True)
    k1, d1 = ex(img)
    ex.profile_enable(False)
    prof = ex.profile_read(reset=True)
    assert prof["resize"][1] == 7 and prof["fast"][1] == 1 and prof["tree"][1] == 1 and prof["desc"][1] == 1
    assert all(prof[s][0] > 0 for s in ("resize", "fast", "tree", "desc"))
    ex.profile_stages(1 << pkg.orbx.STAGES.index("fast"))
    ex.profile_enable(True)
    ex(img); ex(img)
    ex.profile_enable(False)
    prof = ex.profile_read(reset=True)
    ex.profile_stages()
    assert prof["fast"][1] == 2 and prof["fast"][0] > 0
    assert all(prof[s][1] == 0 for s in ("resize", "tree", "desc", "stereo", "stereo_cut"))


def test_single_stream_latency_has_no_cold_lanes():
    """examples/stereo_stream (one camera stream through the pipelined C ABI, the loop of the reference's Examples/Stereo/stereo_kitti.cc:68-117): after
    orbx_pipeline_warm / the first submit every pipeline slot and kernel lane exists, so the FIRST timed frames take what every later frame
    takes (round 3 made a lane per frame inside the timed window: 3-19 ms each against 0.2 ms).  Loose bounds: this is a timing test."""
    import json, os, subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "examples", "stereo_stream")
    if not os.path.exists(exe):
        import __graft_entry__ as ge
        ge.build()
    out = subprocess.run([exe, "--streams", "1", "--frames", "600"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    d = json.loads(out.stdout.strip().splitlines()[-1])
    assert len(d["first_frames_us"]) == 16 and max(d["first_frames_us"]) < 2500, d["first_frames_us"]
    assert d["latency_us_p99"] < 5 * d["latency_us_p50"], d
