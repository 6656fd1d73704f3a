"""k_fast's lane geometry from the host (orbx_fast.hip: fast_lane_entry, the shape classes of orbx_fast_plan) and the LDS-direct tile loads
addressed as scalar base + lane offset (orbx_device.h: lds_load_sbase).

CPU: the exported lane table against a numpy restatement of the formulas the kernel evaluated per wave before, and against what the fields
mean (every pretest group of a row block taken by exactly one lane, masks that cover exactly the detectable pixels), for every detect shape
dw 1..38 x dh 1..40 and both tile pitches.  The tile-load geometry (lane / DWR, lane % DWR) is not tabulated -- the loads it addresses are
what hides the table fetch -- so there is nothing of it to compare.

GPU: extraction stage by stage against the oracle on small images whose cell grids hold the shapes where the lane geometry changes form.
Each case asserts from the cell records (orbx_debug_fast_cells) that the shapes it is there for exist, and from orbx_debug_launch_forms
that the k_fast form it targets ran."""
import numpy as np
import pytest

from tools import synth


# ------------------------------------------------------------------------------------------- CPU: the table

def _model(P, dw, dh):
    """the per-lane set-up k_fast computed in the kernel (one wave per cell), in numpy"""
    lane = np.arange(64, dtype=np.int64)
    gpr = (dw + 3) >> 2
    magic = (0xFFFFFFFF // gpr + 1) & 0xFFFFFFFF
    lq = lane if gpr == 1 else (lane * magic) >> 32
    rpi = min(64 if gpr == 1 else (64 * magic) >> 32, 8)
    lr = np.minimum(lq, rpi)
    gq = lane - lq * gpr
    nvalid = np.clip(dw - 4 * gq, 1, 4)
    vmask = np.where(lr < rpi, 0x80808080 >> (8 * (4 - nvalid)), 0)
    bm_sh = 4 * (gq & 7)
    half_mode = dh <= 32 and dw <= 32
    brow = lane >> 1 if half_mode else lane
    bsh = 16 * (lane & 1) if half_mode else np.zeros(64, np.int64)
    return dict(lq=lq, rpi=rpi, lr=lr, gq=gq, nvalid=nvalid, vmask=vmask, bm_sh=bm_sh, half_mode=half_mode, brow=brow, bsh=bsh,
                pc_off=(lr + 3) * P + 4 * (1 + gq), pb_off=4 * (lr * 2 + (gq >> 3)), row_ok=brow < dh, gpr=gpr)


@pytest.mark.parametrize("P", [48, 80])
def test_lane_table_matches_kernel_formulas(pkg, P):
    for dw in range(1, 39):
        for dh in range(1, 41):
            tab, rpi, half_mode = pkg.orbx.debug_fast_lane_table(P, dw, dh)
            m = _model(P, dw, dh)
            tag = f"P={P} dw={dw} dh={dh}"
            t = tab.astype(np.int64)
            assert rpi == m["rpi"] and half_mode == m["half_mode"], tag
            assert (m["lq"] == np.arange(64) // m["gpr"]).all(), tag          # the magic multiply is the division
            assert (t[:, 0] == m["vmask"]).all(), tag
            assert ((t[:, 1] & 0xFFFF) == m["pc_off"]).all() and ((t[:, 1] >> 16) == m["pb_off"]).all(), tag
            assert ((t[:, 2] & 0xFFFF) == ((m["brow"] << 6) | m["bsh"])).all(), tag
            assert (((t[:, 2] >> 16) & 1) == m["row_ok"]).all(), tag
            assert ((t[:, 2] >> 24) == m["bm_sh"]).all() and ((t[:, 2] >> 17) & 0x7F == 0).all(), tag
            assert (t[:, 3] == 0).all(), tag
            # what the fields mean.  Pretest: the active lanes are the (row, group) pairs of rpi whole rows, each once; the mask bytes
            # of a row's groups are exactly its dw detectable pixels; the bitmap bit of group g of row r is bit 4 g of the row's 64
            act = t[:, 0] != 0
            pairs = set(zip(m["lr"][act].tolist(), m["gq"][act].tolist()))
            assert act.sum() == rpi * m["gpr"] == len(pairs) and pairs == {(r, g) for r in range(rpi) for g in range(m["gpr"])}, tag
            assert 1 <= rpi <= 8 and rpi * m["gpr"] <= 64, tag
            for g in range(m["gpr"]):
                nv = bin(int(t[act & (m["gq"] == g), 0][0])).count("1")
                assert nv == min(4, dw - 4 * g), tag
            bit = (t[:, 1] >> 16) * 8 + (t[:, 2] >> 24)                        # bit offset from the first bitmap row of the iteration
            assert (bit[act] == m["lr"][act] * 64 + 4 * m["gq"][act]).all(), tag
            assert ((t[:, 1] & 0xFFFF)[act] == (m["lr"][act] + 3) * P + 4 + 4 * m["gq"][act]).all(), tag     # tile column 4 = first detectable pixel
            # list: the segments of the existing rows tile the dh x 64 bitmap exactly once
            seg_bits = 16 if half_mode else 64
            ok = ((t[:, 2] >> 16) & 1) == 1
            segs = sorted(zip((t[ok, 2] & 0xFFFF) >> 6, t[ok, 2] & 63))
            want = [(r, b) for r in range(min(dh, 32 if half_mode else 64)) for b in range(0, 32 if half_mode else 64, seg_bits)]
            assert segs == want, tag
            assert dw <= (32 if half_mode else 64) and dh <= (32 if half_mode else 64), tag


def test_lane_table_rejects_bad_shapes(pkg):
    for args in [(64, 30, 30), (48, 0, 30), (48, 39, 30), (48, 30, 0), (80, 60, 30), (48, 30, 65)]:
        with pytest.raises(pkg.OrbxError):
            pkg.orbx.debug_fast_lane_table(*args)


# ------------------------------------------------------------------------------------------- GPU: stage parity on the shapes that matter

def _dense(seed, w, h):
    """binary noise: corners everywhere (dense_corners of test_gpu_parity), so keypoints reach every border the extractor allows"""
    return np.random.default_rng(seed).integers(0, 2, (h, w), dtype=np.uint8) * 255


def _images(kind, seed, w, h, n):
    if kind == "dense":
        return [_dense(seed + i, w, h) for i in range(n)]
    return [synth.image(seed + i, w, h, nshapes=int(w * h / 250) + 40) for i in range(n)]


def _cmp_stage(tag, ex, orc, img, i, kps, desc):
    """image i of the batch just extracted against the oracle, stage by stage (tests/test_gpu_parity.py: _check_stages)"""
    okps, odesc = orc.extract(img)
    for l in range(orc.nlevels):
        g, o = ex.pyramid_level(l, i), orc.level(l)
        assert g.shape == o.shape, f"{tag}: level {l} shape {g.shape} vs {o.shape}"
        bad = np.argwhere(g != o)
        assert len(bad) == 0, f"{tag}: pyramid level {l}: {len(bad)} pixels differ, first at {bad[:3].tolist()}"
    for l in range(orc.nlevels):
        gx, gy, gr = ex.debug_candidates(l, i)
        ox, oy, orr = orc.candidates(l)
        assert len(gx) == len(ox), f"{tag}: level {l}: {len(gx)} FAST candidates vs oracle {len(ox)}"
        assert (gx == ox).all() and (gy == oy).all(), f"{tag}: level {l}: candidate positions/order differ"
        assert (gr == orr).all(), f"{tag}: level {l}: candidate responses differ"
    gc = ex.debug_level_counts(i)
    oc = np.array([orc.nkeypoints(l) for l in range(orc.nlevels)])
    assert (gc == oc).all(), f"{tag}: keypoints per level {gc.tolist()} vs oracle {oc.tolist()}"
    assert len(kps) == len(okps), f"{tag}: {len(kps)} keypoints vs oracle {len(okps)}"
    for f in ("x", "y", "octave", "response", "size", "class_id"):
        bad = np.nonzero(kps[f] != okps[f])[0]
        assert len(bad) == 0, f"{tag}: keypoint field {f} differs at {bad[:5].tolist()}"
    bad = np.nonzero(kps["angle"].view(np.uint32) != okps["angle"].view(np.uint32))[0]
    assert len(bad) == 0, f"{tag}: angle bits differ at {bad[:5].tolist()}"
    bad = np.nonzero((desc != odesc).any(axis=1))[0]
    assert len(bad) == 0, f"{tag}: {len(bad)} descriptors differ, first {bad[:5].tolist()}"
    assert kps.tobytes() == okps.tobytes(), tag
    return okps


# (w, h, levels, level-0 pitch, images, batches, shapes the cell records must hold)
#   last_dw: detect widths of last-column cells; dh: detect heights; tile 48 / 80: the kernel instance (every cell <= 38 px wide or not)
CASES = {
    # last columns 1, 2 and 4 px wide (one pretest group per row, partial or whole), detect heights 28 / 31 (half rows), 34 and 45 (whole rows)
    "1127x100": dict(w=1127, h=100, nl=3, pitch=1128, kind="dense", seed=2, nf=4000, batches=(1, 40, 65), last_dw={1, 2, 4}, dh={28, 31, 34, 45}, tile=48),
    # last columns 3 and 5 px wide (5: two groups, the second with one pixel)
    "942x100": dict(w=942, h=100, nl=2, pitch=944, kind="dense", seed=2, nf=3000, batches=(1, 60, 97), last_dw={3, 5}, dh={28, 34, 45}, tile=48),
    # a last column of 29..31 px (eight groups, the last one partial), detect heights <= 32, 34 and 40 (a fifth pretest iteration);
    # odd level-0 pitch
    "210x150": dict(w=210, h=150, nl=5, pitch=223, kind="scene", seed=9310, nf=600, batches=(1, 120, 216), last_dw=None, dh={34, 40}, tile=48),
    # a cell wider than 38 px on a small level: the 80-byte tile (three rows per load), always one wave per cell on the (cell, image) grid
    "221x230": dict(w=221, h=230, nl=8, pitch=224, kind="scene", seed=9321, nf=500, batches=(1, 9), last_dw=None, dh={34, 40}, tile=80),
}


def _assert_shapes(name, c, cells):
    live = cells[cells[:, 1] == 0]
    dw, dh, th = live[:, 4] - 6, live[:, 5] - 6, live[:, 5]
    last = np.zeros(len(live), bool)            # last column of its level's cell row: the largest ini_x of the level
    for l in np.unique(live[:, 0]):
        s = live[:, 0] == l
        last |= s & (live[:, 2] == live[s, 2].max())
    rpl = 64 // (c["tile"] // 4)
    if c["last_dw"]:
        assert c["last_dw"] <= set(dw[last].tolist()), f"{name}: last-column detect widths {sorted(set(dw[last].tolist()))}"
    else:
        part = [int(v) for v in set(dw[last].tolist()) if 29 <= v <= 32 and v % 4]
        assert part, f"{name}: no last column of 29..32 px with a partial group: {sorted(set(dw[last].tolist()))}"
    assert c["dh"] <= set(dh.tolist()) and (dh <= 32).any(), f"{name}: detect heights {sorted(set(dh.tolist()))}"
    assert (th % rpl == 0).any() and (th % rpl != 0).any(), f"{name}: tile heights {sorted(set(th.tolist()))} against {rpl} rows per load"
    assert (dw.max() <= 38) == (c["tile"] == 48), f"{name}: widest cell {dw.max()}"
    assert c["pitch"] % 64 != 0 and c["pitch"] >= c["w"]
    # one class per distinct shape
    shapes = {}
    for w_, h_, k in zip(dw.tolist(), dh.tolist(), live[:, 7].tolist()):
        assert shapes.setdefault((w_, h_), k) == k, f"{name}: shape {(w_, h_)} in classes {shapes[(w_, h_)]} and {k}"
    assert len(set(shapes.values())) == len(shapes), f"{name}: two shapes share a class: {shapes}"


# k_fast2 (forced) takes a geometry only if every cell is at most 32 px wide: the two wide, low images
@pytest.mark.gpu
@pytest.mark.parametrize("name,pair", [(n, "0") for n in CASES] + [("1127x100", "1"), ("942x100", "1")])
def test_fast_shapes_and_forms(pkg, oracle, monkeypatch, name, pair):
    """every k_fast form the batch size selects (several waves per cell, one wave on the image-major grid, one wave on the (cell, image)
    grid of the 80-byte tile) and, forced, k_fast2, each on cell grids that hold the narrow / partial / tall shapes"""
    import torch
    c = CASES[name]
    monkeypatch.setenv("ORBX_FAST_PAIR", pair)
    w, h, nl, pitch = c["w"], c["h"], c["nl"], c["pitch"]
    nimg = 3
    imgs = _images(c["kind"], c["seed"], w, h, nimg)   # (dense: a seed whose first image has the keypoints asserted at the end)
    orc = oracle.Oracle(c["nf"], 1.2, nl, 20, 7)
    dev = torch.device("cuda", 0)
    bmax = max(c["batches"])
    host = np.zeros((bmax, h, pitch), np.uint8)
    for i in range(bmax):
        host[i, :, :w] = imgs[i % nimg]
    d_img = torch.from_numpy(host).to(dev)
    ex = pkg.ORBextractor(c["nf"], 1.2, nl, 20, 7, device=0, max_size=(w, h), max_batch=bmax)
    cap = ex.max_keypoints(w, h)
    kps = torch.zeros((bmax, cap, 7), dtype=torch.float32, device=dev)
    desc = torch.zeros((bmax, cap, 32), dtype=torch.uint8, device=dev)
    nout = torch.zeros(bmax, dtype=torch.int32, device=dev)
    seen = set()
    okps0 = None
    for B in c["batches"]:
        kps.fill_(-3.0); desc.fill_(0xA5); nout.fill_(-1)
        torch.cuda.synchronize()
        ex.extract_batch_device(d_img.data_ptr(), h * pitch, pitch, B, w, h, kps.data_ptr(), desc.data_ptr(), cap, nout.data_ptr(), None)
        ex.sync()
        f = ex.debug_launch_forms()
        seen.add((f["fast_waves"], f["fast_image_major"]))
        if B == c["batches"][0]:
            _assert_shapes(name, c, ex.debug_fast_cells())
        n = nout.cpu().numpy()
        k = kps.cpu().numpy().view(np.uint8).reshape(bmax, cap, 28)
        d = desc.cpu().numpy()
        for i in sorted({0, B // 2, B - 1}):
            ki = np.frombuffer(k[i, :n[i]].tobytes(), dtype=pkg.KP_DTYPE)
            o = _cmp_stage(f"{name} B={B} image {i} forms {f}", ex, orc, imgs[i % nimg], i, ki, d[i, :n[i]])
            if i == 0:
                okps0 = o
        ref = {}
        for i in range(B):                       # every image of the batch: the final records of its source image
            r = ref.setdefault(i % nimg, (int(n[i]), k[i, :n[i]].tobytes(), d[i, :n[i]].tobytes()))
            assert (int(n[i]), k[i, :n[i]].tobytes(), d[i, :n[i]].tobytes()) == r, f"{name} B={B}: image {i} differs from image {i % nimg}"
    if pair == "1":
        assert seen == {(0, 0)}, f"{name}: k_fast2 was forced, forms seen {seen}"
    elif c["tile"] == 80:
        assert seen == {(1, 0)}, f"{name}: forms seen {seen}"
    else:
        assert {(1, 1)} <= seen and any(nw > 1 for nw, _ in seen) and len(seen) >= 3, f"{name}: k_fast forms seen {seen}"
    if c["kind"] == "dense":
        # k_desc's patch loads (level 0, caller's pitch): the last patch dword ends exactly at the pitch (fast path) and one byte behind it
        # (edge path), and keypoints within 21 px of each border (reflected patches)
        l0 = okps0[okps0["octave"] == 0]
        x, y = l0["x"].astype(np.int64), l0["y"].astype(np.int64)
        assert ((x - 21 + 44) == pitch).any() and ((x - 21 + 44) == pitch + 1).any(), f"{name}: level-0 keypoint columns end at {sorted(set(x.tolist()))[-6:]}"
        assert (x < 21).any() and (x + 21 >= w).any() and (y < 21).any() and (y + 21 >= h).any(), name


@pytest.mark.gpu
def test_resize_tile_tails(pkg, oracle):
    """k_resize's row-group loads: a level of at most 256 columns is one tile that starts at source column 0, so the bytes behind its last
    whole 16-byte piece -- fetched as bytes, not by direct loads -- are the source width mod 16: tails of 1, 13 and 15 bytes and no tail"""
    h, nl = 150, 5
    tails = set()
    for w in (208, 209, 223):
        img = _dense(9300 + w, w, h)
        orc = oracle.Oracle(800, 1.2, nl, 20, 7)
        ex = pkg.ORBextractor(800, 1.2, nl, 20, 7, device=0, max_size=(w, h))
        kps, desc = ex(img)
        okps, odesc = orc.extract(img)
        for l in range(nl):
            g, o = ex.pyramid_level(l), orc.level(l)
            assert g.shape == o.shape and (g == o).all(), f"{w}x{h}: pyramid level {l} differs"
            if l:
                assert o.shape[1] <= 256
                tails.add(orc.level(l - 1).shape[1] % 16)
        assert kps.tobytes() == okps.tobytes() and desc.tobytes() == odesc.tobytes()
    assert {0, 1, 13, 15} <= tails, sorted(tails)
