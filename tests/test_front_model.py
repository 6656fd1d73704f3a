"""Pyramid (ComputePyramid, src/ORBextractor.cc:1345-1394), per-cell FAST (ComputeKeyPointsOctTree, :925-1009), the quadtree cull
(DistributeOctTree, :617-915) and the keypoint records (:1023-1045, :1327-1334) against the independent numpy models of
tests/front_model.py, bit for bit and without a tolerance: the oracle stages on the CPU, the kernels k_pyr*, k_fast, k_fast2 and k_tree on
the GPU, there against the model DIRECTLY.  With orb_model (orientation, rBRIEF) front_model.extract_model is the whole extractor,
so no stage of the headline path is pinned to the oracle alone.

Inputs: textured scenes and directed images (tools/synth.py).  Each directed image exists to reach an edge, and a test asserts ON
THE MODEL'S output and event counts that the edge is reached: suppression that sees zeros outside a cell's own detectable area,
ties that suppress both pixels, the minThFAST pass taken per cell and after suppression, a last cell one pixel wide, a skipped 6-px
column, a 6-px row that is not skipped, and the 2 x 2 mean of an exact halving."""
import numpy as np
import pytest

import front_model as fm
from quadtree_model import quadtree_model
from test_oracle_known_answers import RING, _fast_bruteforce, quadtree_random_sets
from tools import synth

CFG = (500, 1.2, 8, 20, 7)              # the 320 x 240 images: the smallest size at which each of 8 levels still has a cell
CFG_GEOM = (1500, 1.2, 1, 20, 7)        # cell geometry: one level
CFG_HALF = (500, 2.0, 3, 20, 7)         # exact halving
W, H = 320, 240

DIRECTED_320 = ("tie", "straddle", "fallback", "blockchecker")
DIRECTED = DIRECTED_320 + ("geom_813x783", "geom_783x813", "half_482x362", "half_480x362", "half_480x360")
NAMES = DIRECTED + ("scene_320", "scene_640", "lowcontrast", "checker")


def _images():
    yy, xx = np.mgrid[0:480, 0:640]
    return {"tie": (synth.tie_bars()[0], CFG), "straddle": (synth.straddling_corners()[0], CFG), "fallback": (synth.one_cell_fallback()[0], CFG),
            "blockchecker": (synth.block_checkerboard(), CFG),
            "geom_813x783": (synth.image(41, 813, 783), CFG_GEOM), "geom_783x813": (synth.image(42, 783, 813), CFG_GEOM),
            "half_482x362": (synth.image(43, 482, 362), CFG_HALF), "half_480x362": (synth.image(44, 480, 362), CFG_HALF),
            "half_480x360": (synth.image(45, 480, 360), CFG_HALF),
            "scene_320": (synth.image(101, W, H), CFG), "scene_640": (synth.stereo_pair(104, 640, 480)[0], (1000, 1.2, 8, 20, 7)),
            # the two images of test_gpu_parity.py: contrast between minThFAST and iniThFAST; 3-px checks (dense corners)
            "lowcontrast": ((100 + (synth.image(9, 640, 480).astype(np.int32) - 100) // 14).astype(np.uint8), (500, 1.2, 8, 20, 7)),
            "checker": ((((xx // 3 + yy // 3) & 1) * 200 + 20).astype(np.uint8), (800, 1.2, 8, 20, 7))}


@pytest.fixture(scope="module")
def models():
    """per image: the model's records, descriptors (both blur profiles) and per-stage intermediates; computed once, never changed"""
    out = {}
    images = _images()
    assert tuple(images) == NAMES
    for name, (img, cfg) in images.items():
        k, d0, st = fm.extract_model(img, cfg, 0)
        k1, d1, st1 = fm.extract_model(img, cfg, 1, front=st)
        assert k1.tobytes() == k.tobytes()
        out[name] = dict(img=img, cfg=cfg, k=k, d=(d0, d1), st=st, blurred=(st["blurred"], st1["blurred"]))
    return out


def _compare_stages(tag, m, levels, candidates, counts, k, d, profile):
    """`levels`, `candidates`: callables of a level; the first stage that differs from the model names itself"""
    st, cfg = m["st"], m["cfg"]
    for l in range(cfg[2]):
        g = levels(l)
        assert g.shape[::-1] == st["dims"][l], f"{tag}: level {l} is {g.shape[::-1]}, model {st['dims'][l]}"
        bad = np.argwhere(g != st["levels"][l])
        assert len(bad) == 0, f"{tag}: pyramid level {l}: {len(bad)} pixels differ from the model, first at {bad[:3].tolist()}"
    for l in range(cfg[2]):
        gx, gy, gr = candidates(l)
        mx, my, mr = st["candidates"][l]
        assert len(gx) == len(mx), f"{tag}: level {l}: {len(gx)} FAST candidates, model {len(mx)}"
        assert (gx == mx).all() and (gy == my).all(), f"{tag}: level {l}: candidate positions / order differ from the model"
        assert (gr == mr).all(), f"{tag}: level {l}: candidate responses differ from the model"
    assert np.asarray(counts).tolist() == st["counts"].tolist(), f"{tag}: keypoints per level {np.asarray(counts).tolist()}, model {st['counts'].tolist()}"
    assert k.dtype == fm.KP_DTYPE and len(k) == len(m["k"])
    for f in ("x", "y", "octave", "response", "size", "class_id"):
        bad = np.nonzero(k[f] != m["k"][f])[0]
        assert len(bad) == 0, f"{tag}: keypoint field {f} differs from the model at {bad[:5].tolist()} (quadtree selection / order, records)"
    bad = np.nonzero(k["angle"].view(np.uint32) != m["k"]["angle"].view(np.uint32))[0]
    assert len(bad) == 0, f"{tag}: angle bits differ from the model at {bad[:5].tolist()}"
    assert k.tobytes() == m["k"].tobytes(), f"{tag}: records differ from the model"
    bad = np.nonzero((d != m["d"][profile]).any(axis=1))[0]
    assert len(bad) == 0, f"{tag}: blur profile {profile}: {len(bad)} descriptors differ from the model, first {bad[:5].tolist()}"
    assert d.tobytes() == m["d"][profile].tobytes()


# ------------------------------------------------------------------------------------------------ oracle == model, stage by stage

@pytest.mark.parametrize("name", NAMES)
def test_oracle_equals_model(models, oracle, name):
    m = models[name]
    assert oracle.KP_DTYPE == fm.KP_DTYPE
    o = oracle.Oracle(*m["cfg"])
    sf, isf, quota = fm.scale_tables(m["cfg"])
    assert o.scale_factors().tobytes() == sf.tobytes() and o.inv_scale_factors().tobytes() == isf.tobytes()
    assert o.features_per_level().tolist() == quota.tolist()
    h, w = m["img"].shape
    assert fm.level_dims(w, h, m["cfg"]) == m["st"]["dims"]
    for profile in (0, 1):
        o.set_cv_profile(profile)
        k, d = o.extract(m["img"])
        _compare_stages(f"{name} oracle", m, o.level, o.candidates, [o.nkeypoints(l) for l in range(m["cfg"][2])], k, d, profile)
        for l in range(m["cfg"][2]):
            ob, mb = o.level(l, blurred=True), m["blurred"][profile][l]
            assert (ob is None) == (mb is None) and (ob is None or (ob == mb).all()), f"{name}: blurred level {l}, profile {profile}"
    assert (m["d"][0] != m["d"][1]).any()


def test_a_level_without_a_cell_is_rejected(oracle):
    img = synth.image(3, 300, 216)                       # level 7: 84 x 60, 28 px between the borders: no row of cells
    with pytest.raises(ValueError):
        fm.extract_model(img, CFG)
    with pytest.raises(RuntimeError):
        oracle.Oracle(*CFG).extract(img)
    assert fm.level_dims(300, 216, CFG)[7] == (84, 60) and fm.cell_grid(*fm.level_dims(W, H, CFG)[7])["nRows"] == 1


# ------------------------------------------------------------------------------------------------ resize, SURVEY B.2

def test_linear_coefficients_by_hand():
    """6 -> 5 pixels, ratio 1.2: destination d reads source position (d + 0.5) * 1.2 - 0.5 = 0.1, 1.3, 2.5, 3.7, 4.9; the weights
    are cvRound(f * 2048) and cvRound((1 - f) * 2048): 11 bits, 204.8 -> 205, 614.4 -> 614, 1433.6 -> 1434, 1843.2 -> 1843"""
    s, c0, c1 = fm._linear_coeffs(6, 5)
    assert s.tolist() == [0, 1, 2, 3, 4]
    assert c1.tolist() == [205, 614, 1024, 1434, 1843] and c0.tolist() == [1843, 1434, 1024, 614, 205]
    # 3 -> 2 (ratio 1.5): positions 0.25 and 1.75, weights (1536, 512) on pixels (0, 1) and (512, 1536) on pixels (1, 2).  One pixel
    # of 200: t = 200 * a, then >> 4, * b, >> 16, + 2 >> 2.  In the middle every destination weighs it 512 * 512 (12.5 -> 13), in the
    # corner only destination (0, 0) does, 1536 * 1536 (112.5 -> 113)
    assert fm._linear_coeffs(3, 2)[1].tolist() == [1536, 512] and fm._linear_coeffs(3, 2)[2].tolist() == [512, 1536]
    src = np.zeros((3, 3), np.uint8); src[1, 1] = 200
    assert (((512 * ((200 * 512) >> 4)) >> 16) + 2) >> 2 == 13 and (((1536 * ((200 * 1536) >> 4)) >> 16) + 2) >> 2 == 113
    assert fm.resize_model(src, 2, 2).tolist() == [[13, 13], [13, 13]]
    src = np.zeros((3, 3), np.uint8); src[0, 0] = 200
    assert fm.resize_model(src, 2, 2).tolist() == [[113, 0], [0, 0]]
    # 161 -> 80 (ratio 2.0125): positions 0.50625 and 159.49375: 1036.8 -> 1037 and 1011.2 -> 1011; no offset is clamped when shrinking
    s, c0, c1 = fm._linear_coeffs(161, 80)
    assert (s[0], c0[0], c1[0]) == (0, 1011, 1037) and (s[-1], c0[-1], c1[-1]) == (159, 1037, 1011)


@pytest.mark.parametrize("sw,sh,dw,dh", [(72, 60, 60, 50), (300, 144, 250, 120),        # 1.2
                                         (110, 88, 100, 80), (143, 77, 130, 70),        # 1.1
                                         (95, 57, 50, 30), (190, 133, 100, 70),         # 1.9
                                         (161, 161, 80, 80), (322, 161, 160, 80),       # 2.0125
                                         (161, 60, 80, 50), (120, 76, 60, 40), (120, 90, 60, 40),     # 2.0125 by 1.2; exactly 2 by 1.9 and by 2.25: bilinear
                                         (120, 80, 60, 40), (267, 200, 222, 167)])      # exactly 2 by 2: the mean; level 1 -> 2 of 320 x 240
def test_resize_exact(oracle, sw, sh, dw, dh):
    """oracle_resize_linear == resize_model on every pixel: the 11-bit weights, >> 4, >> 16, + 2 >> 2, and which sizes take the mean"""
    rng = np.random.default_rng(sw * 1000 + dh)
    for kind in ("noise", "extremes"):
        src = rng.integers(0, 256, (sh, sw), dtype=np.uint8) if kind == "noise" else (rng.integers(0, 2, (sh, sw)) * 255).astype(np.uint8)
        dst = np.zeros((dh, dw), np.uint8)
        oracle.lib().oracle_resize_linear(src.ctypes.data, sw, sh, sw, dst.ctypes.data, dw, dh, dw)
        exp = fm.resize_model(src, dw, dh)
        bad = np.argwhere(dst != exp)
        assert len(bad) == 0, f"{sw}x{sh} -> {dw}x{dh} {kind}: {len(bad)} pixels differ, first {bad[:3].tolist()}"
    assert fm.takes_mean_path(sw, sh, dw, dh) == ((sw, sh, dw, dh) == (120, 80, 60, 40))


def test_mean_equals_bilinear_at_an_exact_halving():
    """at exactly 2 by 2 every weight is 1024, (a + b) * 1024 >> 4 and * 1024 >> 16 lose nothing, and the bilinear chain IS the rounded
    2 x 2 mean: for cv::resize's switch to INTER_AREA only WHEN it is taken can matter (one axis exactly 2: test_resize_exact,
    test_mean_path_levels), never that it is taken"""
    rng = np.random.default_rng(11)
    for src in (rng.integers(0, 256, (60, 72), dtype=np.uint8), (rng.integers(0, 2, (62, 70)) * 255).astype(np.uint8)):
        h, w = src.shape
        assert fm._linear_coeffs(w, w // 2)[1].tolist() == [1024] * (w // 2) and fm._linear_coeffs(w, w // 2)[0].tolist() == list(range(0, w, 2))
        assert (fm.resize_bilinear(src, w // 2, h // 2) == fm.resize_model(src, w // 2, h // 2)).all()
    # one axis only: the two differ
    s = src.astype(np.int64)                                       # 70 x 62 -> 35 x 30: x is exactly 2, y is not
    mean = (s[0:60:2, 0::2] + s[0:60:2, 1::2] + s[1:60:2, 0::2] + s[1:60:2, 1::2] + 2) >> 2
    assert not fm.takes_mean_path(70, 62, 35, 30) and (fm.resize_model(src, 35, 30) != mean).any()


def test_mean_path_levels(models):
    """scale factor 2.0: which levels are the rounded 2 x 2 mean (both source sizes exactly twice the destination's) and which bilinear"""
    assert models["half_482x362"]["st"]["dims"] == [(482, 362), (241, 181), (120, 90)]
    assert models["half_482x362"]["st"]["mean_path"] == [False, True, False]            # 241 x 181 -> 120 x 90: neither ratio is 2
    assert models["half_480x362"]["st"]["dims"] == [(480, 362), (240, 181), (120, 90)]
    assert models["half_480x362"]["st"]["mean_path"] == [False, True, False]            # 240 -> 120 is exactly 2, 181 -> 90 is not
    assert models["half_480x360"]["st"]["mean_path"] == [False, True, True]
    assert not any(models["scene_320"]["st"]["mean_path"])
    # the two paths do differ on these pixels, so a wrong switch shows
    for name, l in (("half_482x362", 1), ("half_480x360", 2)):
        lv = models[name]["st"]["levels"]
        s = lv[l - 1].astype(np.int64)
        h2, w2 = lv[l].shape
        mean = (s[0:2 * h2:2, 0:2 * w2:2] + s[0:2 * h2:2, 1:2 * w2:2] + s[1:2 * h2:2, 0:2 * w2:2] + s[1:2 * h2:2, 1:2 * w2:2] + 2) >> 2
        assert (lv[l] == mean).all()
    lv = models["half_480x362"]["st"]["levels"]
    s = lv[1].astype(np.int64)
    assert (lv[2] != ((s[0:180:2, 0::2] + s[0:180:2, 1::2] + s[1:180:2, 0::2] + s[1:180:2, 1::2] + 2) >> 2)).mean() > 0.2


# ------------------------------------------------------------------------------------------------ FAST score and the cell grid

def test_fast_raw_score_matches_bruteforce():
    """fast_raw_score on the random 7 x 7 patches of test_fast_score_matches_definition, against its brute force: at threshold t a
    pixel scores its raw score if that is at least t, else it is no corner"""
    rng = np.random.default_rng(5)
    patches = []
    for trial in range(1500):
        base = rng.integers(0, 256)
        patch = np.clip(base + rng.integers(-60, 60, (7, 7)), 0, 255).astype(np.uint8)
        if trial % 3 == 0:
            k0, ln = rng.integers(0, 16), rng.integers(7, 13)
            delta = int(rng.integers(8, 120)) * (1 if rng.random() < 0.5 else -1)
            for k in range(ln):
                dx, dy = RING[(k0 + k) % 16]
                patch[3 + dy, 3 + dx] = np.clip(int(patch[3, 3]) + delta + rng.integers(0, 30) * np.sign(delta), 0, 255)
        patches.append(patch)
    raw = fm.fast_raw_score(np.concatenate(patches, axis=1))[3, 3::7]                     # the centre of every patch
    assert tuple(fm.RING) == tuple(RING)
    hits = 0
    for patch, s in zip(patches, raw.tolist()):
        for t in (7, 20):
            exp = _fast_bruteforce(patch, t)
            assert (s if s >= t else 0) == exp, (patch.tolist(), t, s, exp)
            hits += exp > 0
    assert hits > 100


def test_tie_bars_known_answer(models):
    """two equal neighbours suppress each other; the cell is then empty AFTER suppression, so it runs at minThFAST and finds the weak pixel"""
    m = models["tie"]
    img, meta = synth.tie_bars()
    raw = fm.fast_raw_score(img)
    for a, b in meta["pairs"].values():
        assert raw[a[1], a[0]] == raw[b[1], b[0]] == 214
    assert raw[meta["weak"][1], meta["weak"][0]] == 11
    x, y, r = m["st"]["candidates"][0]
    assert list(zip(x.tolist(), y.tolist(), r.tolist())) == [(54, 54, 11)]
    ev = m["st"]["events"][0]
    assert ev["first_corners"][1, 1] == 2 and ev["first_corners"][1, 3] == 2 and ev["first_corners"][1, 5] == 4
    assert ev["emptied"] == 3 and ev["kept"].sum() == 1 and ev["kept"][1, 1] == 1
    assert ev["tie_suppressed"] == 16                                                     # 8 pixels, in both passes of their cells
    assert (ev["state"] == fm.CELL_SECOND_PASS).all()                                     # every other cell is flat


def test_straddling_corners_reach_the_boundaries(models):
    m = models["straddle"]
    _, meta = synth.straddling_corners()
    x, y, _ = m["st"]["candidates"][0]
    got = set(zip((x + 16).tolist(), (y + 16).tolist()))
    for weak, strong in meta["across"]:
        assert weak in got and strong in got, (weak, strong)                             # both kept: a cell boundary runs between them
    for weak, strong in meta["inside"]:
        assert weak not in got and strong in got, (weak, strong)                         # inside a cell the weaker one goes
    for l in (0, 1):
        bk = m["st"]["events"][l]["border_kept"]
        kinds = dict(vertical=sum(1 for b in bk if b[2] and not b[3]), horizontal=sum(1 for b in bk if b[3] and not b[2]),
                     corner=sum(1 for b in bk if b[2] and b[3]))
        assert all(v >= 2 for v in kinds.values()), f"level {l}: {kinds}"
    assert len(m["st"]["events"][0]["border_kept"]) == len(meta["across"])


def test_one_cell_fallback_is_isolated(models):
    """the minThFAST pass is decided per cell: each low-contrast cell takes it, none of its 8 neighbours does, and it finds corners"""
    m = models["fallback"]
    _, cells = synth.one_cell_fallback()
    ev = m["st"]["events"][0]
    second = ev["state"] == fm.CELL_SECOND_PASS
    assert sorted(map(tuple, np.argwhere(second).tolist())) == sorted(cells)
    for i, j in cells:
        assert 0 < i < second.shape[0] - 1 and 0 < j < second.shape[1] - 1
        assert second[i - 1:i + 2, j - 1:j + 2].sum() == 1
        assert (ev["kept"][i - 1:i + 2, j - 1:j + 2] > 0).all() and ev["first_corners"][i, j] == 0
    # whole frames of fallback, and cells that fall back only after suppression
    assert all((e["state"] == fm.CELL_SECOND_PASS).sum() > e["state"].size // 2 for e in models["lowcontrast"]["st"]["events"])
    assert models["checker"]["st"]["events"][0]["emptied"] > 100


def test_cell_geometry_edges(models):
    """783 px: a last cell 7 px wide (high) with one detectable column (row); 813 px: a 6-px remainder that is skipped as a column
    (iniX >= maxBorderX - 6) and NOT skipped as a row (iniY >= maxBorderY - 3 is false): it runs both passes on nothing"""
    a, b = models["geom_813x783"]["st"]["events"][0], models["geom_783x813"]["st"]["events"][0]
    for ev, wide in ((a, True), (b, False)):
        g = ev["grid"]
        assert (g["wCell"], g["hCell"]) == (31, 31) and (g["nCols"], g["nRows"]) == ((26, 25) if wide else (25, 26))
    # 813 wide: column 25 skipped; 783 high: row 24 is 7 px high
    assert (a["state"][:, 25] == fm.CELL_SKIPPED_COL).all() and (a["state"][:, :25] != fm.CELL_SKIPPED_COL).all()
    assert a["grid"]["maxBorderX"] - (16 + 25 * 31) == 6
    assert ((a["roi"][24, :25, 3] - a["roi"][24, :25, 2]) == 7).all() and a["kept"][24].sum() >= 3
    # 783 wide: column 24 is 7 px wide; 813 high: row 25 is 6 px high, not skipped, second pass, nothing found
    assert ((b["roi"][:25, 24, 1] - b["roi"][:25, 24, 0]) == 7).all() and b["kept"][:, 24].sum() >= 3
    assert ((b["roi"][25, :, 3] - b["roi"][25, :, 2]) == 6).all()
    assert (b["state"][25] == fm.CELL_SECOND_PASS).all() and b["kept"][25].sum() == 0 and b["first_corners"][25].sum() == 0
    assert not (a["state"] == fm.CELL_SKIPPED_ROW).any() and not (b["state"] == fm.CELL_SKIPPED_ROW).any()
    # candidates of a one-column cell sit on that column
    x, y, _ = models["geom_783x813"]["st"]["candidates"][0]
    assert (x == 24 * 31 + 3).sum() == b["kept"][:, 24].sum() and x.max() == 24 * 31 + 3


def test_event_floors(models):
    """the suppression edges are reached in numbers, not by luck.  Floors are near half of what the model measured (in brackets)"""
    s = models["scene_320"]["st"]["events"]
    assert sum(len(e["border_kept"]) for e in s) >= 150                 # [298] kept only because the stronger neighbour is outside the cell
    assert sum(e["tie_suppressed"] for e in s) >= 330                   # [664] suppressed by an equal neighbour
    c = models["blockchecker"]["st"]["events"]
    assert sum(e["emptied"] for e in c) >= 26                           # [53] cells whose first pass had corners and kept none
    assert sum(len(e["border_kept"]) for e in models["scene_640"]["st"]["events"]) >= 430      # [869]
    assert sum(e["tie_suppressed"] for e in models["geom_813x783"]["st"]["events"]) >= 600     # [1258]


# ------------------------------------------------------------------------------------------------ quadtree

def _oracle_tree(oracle, xs, ys, r, box, N):
    xs = np.ascontiguousarray(xs, np.int32); ys = np.ascontiguousarray(ys, np.int32); r = np.ascontiguousarray(r, np.int32)
    out = np.zeros(len(xs) + 1, np.int32)
    cnt = oracle.lib().oracle_distribute_octtree(xs.ctypes.data, ys.ctypes.data, r.ctypes.data, len(xs), *box, N, out.ctypes.data, len(out))
    return out[:cnt].tolist()


def test_quadtree_three_ways_random(oracle):
    """the sequential model (a list, as the reference) == the oracle == the kernel's data-parallel formulation"""
    reached = dict(breaks=0, equal_counts=0, leaf_ties=0, sorted_passes=0, two_roots=0)
    for trial, w, h, xs, ys, r, N in quadtree_random_sets():
        box = (16, 16 + w, 16, 16 + h)
        info = {}
        seq = fm.distribute_octtree_model(xs, ys, r, *box, N, info=info).tolist()
        assert seq == _oracle_tree(oracle, xs, ys, r, box, N), trial
        assert seq == quadtree_model(xs, ys, r, *box, N).tolist(), trial
        reached["breaks"] += sum(1 for j in info["breaks"] if j > 0); reached["equal_counts"] += info["equal_counts"]
        reached["leaf_ties"] += info["leaf_ties"]; reached["sorted_passes"] += info["sorted_passes"]; reached["two_roots"] += info["live_roots"] > 1
    assert all(v >= 20 for v in reached.values()), reached


def _tree_case(oracle, pts, box, N):
    xs, ys, r = (np.array(v) for v in zip(*pts))
    info = {}
    seq = fm.distribute_octtree_model(xs, ys, r, *box, N, info=info).tolist()
    assert seq == _oracle_tree(oracle, xs, ys, r, box, N) == quadtree_model(xs, ys, r, *box, N).tolist()
    return seq, info


def test_quadtree_directed(oracle):
    box = (16, 116, 16, 116)                                     # 100 x 100: one root; halves 50, 25, 13 (ceil of 12.5), 7 (ceil of 6.5)
    # one point per quadrant, N = 0: one sweep; the children are pushed to the FRONT in the order n1 .. n4
    seq, info = _tree_case(oracle, [(10, 10, 9), (60, 10, 9), (10, 60, 9), (60, 60, 9)], box, 0)
    assert seq == [3, 2, 1, 0] and info["sweeps"] == 1
    # one point
    assert _tree_case(oracle, [(40, 40, 9)], box, 10)[0] == [0]
    # a response tie inside a leaf: the first one wins (strict >); all three fall into n1, so the list does not grow and the loop ends
    seq, info = _tree_case(oracle, [(10, 10, 30), (12, 10, 30), (11, 12, 20)], box, 1)
    assert seq == [0] and info["leaf_ties"] == 1
    # the boundary belongs to the right child (<), and each new pair of children goes to the front.  [0, 100) splits at 50: {49} | {50, 74,
    # 75}; 2 + 3 > 4, so by count: [50, 100) splits at 75: {50, 74} | {75}; [50, 75) splits at 50 + ceil(12.5) = 63: {50} | {74}
    seq, _ = _tree_case(oracle, [(49, 0, 9), (50, 0, 9), (74, 0, 8), (75, 0, 7)], box, 4)
    assert seq == [2, 1, 3, 0]
    # half of 25 is 13, not 12: [0, 25) splits into {12} | {13}.  By floor both would fall right of 12, the list would not grow, and the
    # loop would end with three leaves [0, 2, 3]
    seq, _ = _tree_case(oracle, [(12, 0, 9), (13, 0, 8), (30, 0, 7), (60, 0, 6)], box, 4)
    assert seq == [1, 0, 2, 3]
    # N reached in the middle of a back-to-front sweep, among nodes of equal count: four quadrants of 3 points each, N = 7.  After
    # the first sweep 4 nodes (4 + 3 * 4 > 7): sorted by (count, creation), all counts equal, so the LAST created quadrant (n4, lower
    # right) splits first (4 -> 6 nodes), then n3 (-> 8 >= 7): break with 2 nodes left unsplit
    quad = lambda ox, oy: [(ox + 5, oy + 5, 10), (ox + 30, oy + 5, 11), (ox + 5, oy + 30, 12)]
    pts = quad(0, 0) + quad(50, 0) + quad(0, 50) + quad(50, 50)
    seq, info = _tree_case(oracle, pts, box, 7)
    assert info["breaks"] == [2] and info["equal_counts"] == 1 and info["sorted_passes"] == 1
    assert seq == [8, 7, 6, 11, 10, 9, 5, 2]                    # n3's children (pushed last) lead, then n4's, then the unsplit n2, n1
    # ascending counts instead: the fullest node splits first
    pts = quad(0, 0) + [(40, 40, 3)] + quad(50, 0) + quad(0, 50) + quad(50, 50)
    seq, info = _tree_case(oracle, pts, box, 6)
    assert info["breaks"] == [3] and seq == [3, 2, 1, 0, 12, 9, 6]    # only n1 (4 points, created first) was split: 4 - 1 + 4 = 7 nodes
    # all points in one root of two (200 x 100: nIni = 2, hX = 100); the empty root is erased
    box2 = (16, 216, 16, 116)
    seq, info = _tree_case(oracle, [(110, 10, 9), (160, 10, 9), (110, 60, 9), (160, 60, 9)], box2, 4)
    assert info["roots"] == 2 and info["live_roots"] == 1 and seq == [3, 2, 1, 0]
    # the root is kp.pt.x / hX, truncated: 250 x 100 rounds to 3 roots (2.5 rounds away from zero) of 83.33: x = 83 is root 0, 84 root 1
    seq, info = _tree_case(oracle, [(83, 10, 9), (84, 10, 9), (166, 10, 9), (167, 10, 9)], (16, 266, 16, 116), 0)
    assert info["roots"] == 3 and info["live_roots"] == 3       # roots 0 and 2 hold one point each; root 1 = [83, 166) splits at 83 + 42
    assert seq == [2, 1, 0, 3]


def test_model_levels_use_both_tree_phases(models):
    """the quadtree edges are reached inside the extractor too: re-run the model's cull on its own candidates"""
    m = models["scene_640"]
    quota = fm.scale_tables(m["cfg"])[2]
    breaks = ties = 0
    for l in range(m["cfg"][2]):
        x, y, r = m["st"]["candidates"][l]
        g = m["st"]["events"][l]["grid"]
        info = {}
        keep = fm.distribute_octtree_model(x, y, r, g["minBorderX"], g["maxBorderX"], g["minBorderY"], g["maxBorderY"], int(quota[l]), info=info)
        assert keep.tolist() == m["st"]["keep"][l].tolist()
        breaks += sum(1 for j in info["breaks"] if j > 0); ties += info["leaf_ties"]
    assert breaks >= 4 and ties >= 20, (breaks, ties)


# ------------------------------------------------------------------------------------------------ records

def test_record_fields(models):
    """:1023 size = int(31 * scale) truncated; :1041 + minBorder; :1327-1334 the level coordinates times the fp32 scale factor"""
    m = models["scene_320"]
    sf = fm.scale_tables(CFG)[0]
    assert [int(np.float32(31) * s) for s in sf] == [31, 37, 44, 53, 64, 77, 92, 111]     # 1.2^4 * 31 = 64.28, 1.2^6 * 31 = 92.57: rounding gives 93
    k, off = m["k"], 0
    for l in range(8):
        n = int(m["st"]["counts"][l])
        x, y, r = m["st"]["candidates"][l]
        keep = m["st"]["keep"][l]
        part = k[off:off + n]
        assert (part["octave"] == l).all() and (part["size"] == int(np.float32(31) * sf[l])).all()
        scale = sf[l] if l else np.float32(1)
        assert (part["x"] == (x[keep] + 16).astype(np.float32) * scale).all() and (part["y"] == (y[keep] + 16).astype(np.float32) * scale).all()
        assert (part["response"] == r[keep]).all()
        off += n
    assert off == len(k)
    # (float)x * (float)scale is exact in double, so promoting the operands changes nothing; a scale table kept in double does
    lx = np.concatenate([m["st"]["level_xy"][l][0] for l in range(1, 8)]); lv = k["octave"][k["octave"] > 0]
    dbl = (lx * np.float64(np.float32(1.2)) ** lv).astype(np.float32)
    assert (dbl != k["x"][k["octave"] > 0]).any()


# ------------------------------------------------------------------------------------------------ GPU: HIP == model, directly

def _hip_stages(tag, ex, m, profile, image_index=0, k=None, d=None):
    if k is None:
        k, d = ex(m["img"])
    _compare_stages(tag, m, lambda l: ex.pyramid_level(l, image_index), lambda l: ex.debug_candidates(l, image_index),
                    ex.debug_level_counts(image_index), k, d, profile)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_hip_equals_model(pkg, models, name):
    m = models[name]
    h, w = m["img"].shape
    ex = pkg.ORBextractor(*m["cfg"], device=0, max_size=(w, h))
    _hip_stages(f"{name} HIP", ex, m, 0)
    ex.set_cv_profile(pkg.orbx.CV_PROFILE_3_4_2)
    _hip_stages(f"{name} HIP, blur profile 3.4.2", ex, m, 1)


def _cell_widths(w, cfg):
    return [fm.cell_grid(lw, 100)["wCell"] for lw, _ in fm.level_dims(w, 100, cfg)]


@pytest.fixture(scope="module")
def models_few_levels():
    """the directed 320 x 240 images with 2 levels and with 1.  With 8 levels the top level is a single cell 57 px wide, and a geometry
    with a cell wider than 38 px runs the general k_fast, one wave per cell, whatever is asked for; 2 levels (cells of 32 and 34 px)
    take the waves-per-cell forms, 1 level (32 px) also admits the pair kernel"""
    out = {}
    for nl in (1, 2):
        cfg = (CFG[0], CFG[1], nl) + CFG[3:]
        for name in DIRECTED_320:
            img = _images()[name][0]
            k, d, st = fm.extract_model(img, cfg, 0)
            out[name, nl] = dict(img=img, cfg=cfg, k=k, d=(d, None), st=st)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["pair0", "pair1", "waves1", "waves2", "waves3", "waves4", "groups0", "groups64"])
def test_hip_forms_on_directed_images(pkg, models, models_few_levels, monkeypatch, form):
    """every launch form of the front stages on the directed 320 x 240 images: k_fast / k_fast2, 1..4 waves per cell, one pyramid
    launch per level / several levels per launch; with 8, 2 and 1 levels, and the form that really ran is asserted"""
    if form.startswith("pair"):
        monkeypatch.setenv("ORBX_FAST_PAIR", form[4:]); monkeypatch.setenv("ORBX_FAST_WAVES", "1")
    elif form.startswith("waves"):
        monkeypatch.setenv("ORBX_FAST_WAVES", form[5:])
    assert max(_cell_widths(W, CFG)) == 57 and _cell_widths(W, CFG)[:2] == [32, 34]
    for nl in (8, 2, 1):
        cfg = (CFG[0], CFG[1], nl) + CFG[3:]
        ex = pkg.ORBextractor(*cfg, device=0, max_size=(W, H))
        if form.startswith("groups"):
            ex.set_pyramid_group_limit(int(form[6:]))
        for name in DIRECTED_320:
            _hip_stages(f"{name} {form}, {nl} levels", ex, models[name] if nl == 8 else models_few_levels[name, nl], 0)
            assert ex.debug_fast_form() == (2 if form == "pair1" and nl == 1 else 1), (form, nl, ex.debug_fast_form())
            if form.startswith("waves"):
                assert ex.debug_launch_forms()["fast_waves"] == (1 if nl == 8 else int(form[5:])), (form, nl)


@pytest.mark.gpu
def test_hip_batch_of_directed_images_equals_model(pkg, models):
    """all directed 320 x 240 images in one orbx_extract_batch_device launch into poisoned buffers; levels, candidates and counts of
    every image of the batch are read back by image_index"""
    import torch
    names = DIRECTED_320
    B = len(names)
    dev = torch.device("cuda", 0)
    pitch = (W + 63) // 64 * 64
    host = np.zeros((B, H, pitch), np.uint8)
    for i, name in enumerate(names):
        host[i, :, :W] = models[name]["img"]
    imgs = torch.from_numpy(host).to(dev)
    ex = pkg.ORBextractor(*CFG, device=0, max_size=(W, H), max_batch=B)
    cap = ex.max_keypoints(W, H)
    kps = torch.full((B, cap, 7), -3.0, dtype=torch.float32, device=dev)
    desc = torch.full((B, cap, 32), 0xA5, dtype=torch.uint8, device=dev)
    nout = torch.full((B,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ex.extract_batch_device(imgs.data_ptr(), H * pitch, pitch, B, W, H, kps.data_ptr(), desc.data_ptr(), cap, nout.data_ptr(), None)
    ex.sync()
    n = nout.cpu().numpy(); k_h = kps.cpu().numpy().view(np.uint8).reshape(B, cap, 28); d_h = desc.cpu().numpy()
    for i, name in enumerate(names):
        m = models[name]
        assert n[i] == len(m["k"]), f"{name}: {n[i]} keypoints, model {len(m['k'])}"
        k = np.frombuffer(k_h[i, :n[i]].tobytes(), dtype=fm.KP_DTYPE)
        _hip_stages(f"batch {name}", ex, m, 0, image_index=i, k=k, d=d_h[i, :n[i]])
