"""Orientation (IC_Angle, src/ORBextractor.cc:83-111) and steered BRIEF (computeOrbDescriptor, :116-157) against the independent numpy
models of tests/orb_model.py, bit for bit: the oracle stages ic_angle / orb_descriptor on the CPU, the kernel k_desc on the GPU.

Inputs: two textured scenes and four directed 320 x 240 images (tools/synth.py: isolated_dots, dots_with_bar, border_lattice,
block_checkerboard).  Each directed image exists to reach an edge, and a test asserts on the oracle's output that the edge is reached:
orientations of exactly 0 / 90 / 180 / 270 degrees, keypoints on the first and last admissible column and row of levels 0..3, and
compared pixel pairs that are equal (t0 < t1 must give 0)."""
import numpy as np
import pytest

import orb_model
from tools import synth

CFG = (500, 1.2, 8, 20, 7)          # the directed images: 8 levels, scale factor 1.2, 500 features
W, H = 320, 240


def _images():
    left = synth.stereo_pair(104, 640, 480)[0]
    return {"dots": (synth.isolated_dots()[0], CFG), "bars": (synth.dots_with_bar()[0], CFG), "lattice": (synth.border_lattice(), CFG),
            "checker": (synth.block_checkerboard(), CFG), "scene_320": (synth.image(101, W, H), CFG), "scene_640": (left, (1000, 1.2, 8, 20, 7))}


DIRECTED = ("dots", "bars", "lattice", "checker")
NAMES = DIRECTED + ("scene_320", "scene_640")


@pytest.fixture(scope="module")
def cases(oracle):
    """per image: the oracle's keypoints and descriptors, and the model's angles and descriptors for the same keypoints"""
    out = {}
    images = _images()
    assert tuple(images) == NAMES
    for name, (img, cfg) in images.items():
        o = oracle.Oracle(*cfg)
        k, d = o.extract(img)
        angles, desc, info = orb_model.extract_tail_model(o, k)
        out[name] = dict(img=img, cfg=cfg, k=k, d=d, angles=angles, desc=desc, info=info,
                         dims=[o.level(l).shape[::-1] for l in range(cfg[2])])
    return out


def _axis_angles(oracle):
    """what fastAtan2 returns on the four half-axes: its own constants"""
    return {0: oracle.fast_atan2(0, 1), 90: oracle.fast_atan2(1, 0), 180: oracle.fast_atan2(0, -1), 270: oracle.fast_atan2(-1, 0)}


def _count(angles, value):
    return int((angles.view(np.uint32) == np.float32(value).view(np.uint32)).sum())


def test_umax_model_equals_oracle(oracle):
    assert orb_model.umax_model().tolist() == oracle.Oracle(*CFG).umax().tolist() == [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]


def test_pattern_fixture_is_the_oracle_table(oracle):
    """the model reads the reference-pinned fixture; a descriptor match below then also pins the oracle's copy of the table"""
    p = orb_model.load_pattern()
    assert p.shape == (512, 2) and p[0].tolist() == [8, -3] and p[1].tolist() == [9, 5] and np.abs(p).max() <= 15


@pytest.mark.parametrize("name", NAMES)
def test_oracle_equals_model(cases, name):
    c = cases[name]
    assert len(c["k"]) > 100
    bad = np.nonzero(c["k"]["angle"].view(np.uint32) != c["angles"].view(np.uint32))[0]
    assert len(bad) == 0, f"{name}: angle differs at {bad[:5].tolist()}: oracle {c['k']['angle'][bad[:5]]} model {c['angles'][bad[:5]]}"
    bad = np.nonzero((c["d"] != c["desc"]).any(axis=1))[0]
    assert len(bad) == 0, f"{name}: {len(bad)} descriptors differ, first {bad[:5].tolist()}"
    assert c["d"].tobytes() == c["desc"].tobytes() and c["k"]["angle"].tobytes() == c["angles"].tobytes()


def test_directed_images_reach_their_edges(cases, oracle):
    ax = _axis_angles(oracle)
    assert [float(ax[a]) for a in (0, 90, 180, 270)] == [0.0, 90.0, 180.0, 270.0]
    # isolated dots: m10 = m01 = 0, fastAtan2(0, 0) = 0
    assert _count(cases["dots"]["k"]["angle"], ax[0]) >= 5
    # one bar on an axis: each of the four axis orientations, exactly
    n_axis = {a: _count(cases["bars"]["k"]["angle"], v) for a, v in ax.items()}
    assert all(n >= 5 for n in n_axis.values()), n_axis
    # the first and last admissible keypoint column and row of levels 0..3
    c = cases["lattice"]
    for l in range(4):
        m = c["k"]["octave"] == l
        lx, ly = c["info"]["level_x"][m], c["info"]["level_y"][m]
        w, h = c["dims"][l]
        got = dict(x19=int((lx == 19).sum()), xlast=int((lx == w - 20).sum()), y19=int((ly == 19).sum()), ylast=int((ly == h - 20).sum()))
        assert all(v >= 1 for v in got.values()), f"level {l} ({w} x {h}): {got}"
    # equal pixels in compared pairs
    assert cases["checker"]["info"]["equal_pairs"] >= 1000, cases["checker"]["info"]["equal_pairs"]
    blur_ends = cases["checker"]["img"]
    assert blur_ends.min() == 0 and blur_ends.max() == 255


# ------------------------------------------------------------------------------------------------ GPU

def _check_against_both(tag, k, d, c):
    """HIP output against the oracle (whole records) and against the model directly (angles and descriptors)"""
    assert len(k) == len(c["k"]), f"{tag}: {len(k)} keypoints vs oracle {len(c['k'])}"
    assert k.tobytes() == c["k"].tobytes(), f"{tag}: keypoint records differ from the oracle"
    assert d.tobytes() == c["d"].tobytes(), f"{tag}: descriptors differ from the oracle"
    bad = np.nonzero(k["angle"].view(np.uint32) != c["angles"].view(np.uint32))[0]
    assert len(bad) == 0, f"{tag}: angle differs from the model at {bad[:5].tolist()}: {k['angle'][bad[:5]]} vs {c['angles'][bad[:5]]}"
    bad = np.nonzero((d != c["desc"]).any(axis=1))[0]
    assert len(bad) == 0, f"{tag}: {len(bad)} descriptors differ from the model, first {bad[:5].tolist()}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_hip_equals_model_and_oracle(pkg, cases, name):
    c = cases[name]
    h, w = c["img"].shape
    ex = pkg.ORBextractor(*c["cfg"], device=0, max_size=(w, h))
    k, d = ex(c["img"])
    _check_against_both(name, k, d, c)


@pytest.mark.gpu
def test_hip_batch_of_directed_images(pkg, cases):
    """all directed images in one orbx_extract_batch_device launch (the batch size selects other launch forms), into poisoned buffers"""
    import torch
    B = len(DIRECTED)
    dev = torch.device("cuda", 0)
    pitch = (W + 63) // 64 * 64
    host = np.zeros((B, H, pitch), np.uint8)
    for i, name in enumerate(DIRECTED):
        host[i, :, :W] = cases[name]["img"]
    imgs = torch.from_numpy(host).to(dev)
    ex = pkg.ORBextractor(*CFG, device=0, max_size=(W, H), max_batch=B)
    cap = ex.max_keypoints(W, H)
    kps = torch.full((B, cap, 7), -3.0, dtype=torch.float32, device=dev)        # poisoned: everything below a count must be rewritten
    desc = torch.full((B, cap, 32), 0xA5, dtype=torch.uint8, device=dev)
    nout = torch.full((B,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ex.extract_batch_device(imgs.data_ptr(), H * pitch, pitch, B, W, H, kps.data_ptr(), desc.data_ptr(), cap, nout.data_ptr(), None)
    ex.sync()
    n = nout.cpu().numpy(); k_h = kps.cpu().numpy().view(np.uint8).reshape(B, cap, 28); d_h = desc.cpu().numpy()
    for i, name in enumerate(DIRECTED):
        c = cases[name]
        assert n[i] == len(c["k"]), f"{name}: {n[i]} keypoints vs oracle {len(c['k'])}"
        k = np.frombuffer(k_h[i, :n[i]].tobytes(), dtype=c["k"].dtype)
        _check_against_both(f"batch {name}", k, d_h[i, :n[i]], c)
