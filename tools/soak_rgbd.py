"""Randomized parity soak of the RGB-D forms (include/orbx.h: orbx_extract_rgbd, _submit / _wait, orbx_rgbd_depth_batch_device) against the
numpy restatement of tests/test_rgbd.py on the C oracle's keypoints and undistorted positions: random geometry, depth scale, depth type,
distortion on / off, grey / colour input, batch size, both depth transports, RGB-D tickets interleaved with mono tickets.
Run on the GPU box: python tools/soak_rgbd.py [seconds] [seed] [out]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import __graft_entry__ as ge  # noqa: E402
from oracle import oracle_py as O  # noqa: E402
from tools import synth  # noqa: E402
import test_rgbd as T  # noqa: E402

f32 = np.float32
pkg = ge.load_pkg()
budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 11
out = sys.argv[3] if len(sys.argv) > 3 else None
rng = np.random.Generator(np.random.PCG64(seed))
SIZES = [(640, 480), (320, 240), (752, 480), (1241, 376)]
handles = {}


def handle(w, h, gather, batch=2):
    key = (w, h, gather, batch)
    if key not in handles:
        os.environ["ORBX_PIPE_RGBD_GATHER"] = "1" if gather else "0"
        handles[key] = pkg.ORBextractor(1000, 1.2, 8, 20, 7, device=0, max_size=(w, h), max_batch=batch)
        os.environ.pop("ORBX_PIPE_RGBD_GATHER")
    return handles[key]


def frame(w, h, t):
    ch = int(rng.choice([1, 3, 4]))
    img = synth.image(t, w, h) if ch == 1 else np.stack([synth.image(t + 31 * c, w, h) for c in range(ch)], 2)
    rgb = bool(rng.integers(0, 2))
    gray = img if ch == 1 else T._gray_of(img, rgb)
    if rng.random() < 0.5:
        raw = rng.integers(0, 65536, (h, w)).astype(np.uint16); raw[rng.random((h, w)) < 0.1] = 0
    else:
        raw = rng.uniform(-1, 8, (h, w)).astype(f32); raw[rng.random((h, w)) < 0.02] = np.nan; raw[rng.random((h, w)) < 0.01] = np.inf
    return img, rgb, gray, raw


t0 = time.time(); trial = 0; frames = 0
while time.time() - t0 < budget:
    trial += 1
    w, h = SIZES[int(rng.integers(0, len(SIZES)))]
    dist = [0.0] * 5 if rng.random() < 0.3 else [float(rng.uniform(-0.3, 0.3)), float(rng.uniform(-0.9, 0.9)), float(rng.uniform(-0.01, 0.01)),
                                                  float(rng.uniform(-0.01, 0.01)), float(rng.uniform(-1, 1.2))][:int(rng.choice([4, 5]))]
    scale = float(rng.choice([1.0, 1.000005, 1.00002, 1 / 5000, 1 / 5208, 0.001]))
    bf = float(rng.uniform(20, 400))
    fx, fy = float(rng.uniform(300, 700)), float(rng.uniform(300, 700))
    p = pkg.RGBDParams(fx, fy, w / 2 + float(rng.normal(0, 5)), h / 2 + float(rng.normal(0, 5)), dist, bf, depth_scale=scale)
    gather = bool(rng.integers(0, 2))
    ex = handle(w, h, gather)
    nf = int(rng.integers(1, 7))
    fr = [frame(w, h, 10000 * seed + 100 * trial + i) for i in range(nf)]
    exp = []
    for img, rgb, gray, raw in fr:
        k, d = O.Oracle(1000, 1.2, 8, 20, 7).extract(gray)
        xy = np.stack([k["x"], k["y"]], 1).astype(f32)
        if dist[0] != 0:
            xy = O.undistort_points(xy, fx, fy, p.cx, p.cy, dist)
        ur, z = T.restate(k["x"], k["y"], xy[:, 0], raw, p.depth_scale, bf)
        exp.append((k, d, xy, ur, z))
    tag = f"trial {trial} {w}x{h} dist {len(dist)}/{dist[0] != 0} scale {scale} gather {gather}"
    for i, (img, rgb, gray, raw) in enumerate(fr):      # one call
        T._check_frame(tag + f" one-call {i}", ex.extract_rgbd(img, raw, p, rgb=rgb), exp[i])
    depth = int(rng.integers(1, 5))                      # pipelined, mono tickets in between
    q, got = [], {}
    mono = synth.image(trial, w, h)
    emono = ex(mono)
    for i, (img, rgb, gray, raw) in enumerate(fr):
        q.append((i, ex.extract_rgbd_submit(img, raw, p, rgb=rgb)))
        if rng.random() < 0.3 and len(q) < depth:
            q.append((None, ex.extract_submit(mono)))
        while len(q) >= depth:
            j, t = q.pop(0)
            if j is None:
                assert ex.extract_wait(t)[0].tobytes() == emono[0].tobytes(), tag
            else:
                got[j] = ex.extract_rgbd_wait(t)
    for j, t in q:
        if j is None:
            assert ex.extract_wait(t)[0].tobytes() == emono[0].tobytes(), tag
        else:
            got[j] = ex.extract_rgbd_wait(t)
    for i in range(nf):
        T._check_frame(tag + f" pipelined {i} depth {depth}", got[i], exp[i])
    grey = [g for _, _, g, raw in fr if raw.dtype == fr[0][3].dtype]    # batched device form: one depth type per launch
    raws = [raw for _, _, g, raw in fr if raw.dtype == fr[0][3].dtype]
    idx = [i for i in range(nf) if fr[i][3].dtype == fr[0][3].dtype]
    import torch
    exb = handle(w, h, False, batch=8)
    dev = torch.device("cuda", 0)
    B = len(grey)
    pitch = (w + 63) // 64 * 64
    host = np.zeros((B, h, pitch), np.uint8)
    for i, g in enumerate(grey):
        host[i, :, :w] = g
    timg = torch.from_numpy(host).to(dev); tdep = torch.from_numpy(np.stack(raws)).to(dev)
    cap = exb.max_keypoints(w, h)
    kps = torch.zeros((B, cap, 7), dtype=torch.float32, device=dev); desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device=dev)
    n = torch.zeros(B, dtype=torch.int32, device=dev)
    ur = torch.full((B, cap), 9.0, dtype=torch.float32, device=dev); z = torch.full((B, cap), 9.0, dtype=torch.float32, device=dev)
    xy = torch.full((B, cap, 2), 9.0, dtype=torch.float32, device=dev)
    st = torch.cuda.Stream(device=dev)
    es = raws[0].itemsize
    exb.extract_batch_device(timg.data_ptr(), h * pitch, pitch, B, w, h, kps.data_ptr(), desc.data_ptr(), cap, n.data_ptr(), st.cuda_stream)
    pkg.rgbd_depth_batch_device(0, kps.data_ptr(), n.data_ptr(), cap, B, tdep.data_ptr(), h * w * es, w * es, w, h, p,
                                pkg.DEPTH_U16 if es == 2 else pkg.DEPTH_F32, ur.data_ptr(), z.data_ptr(), xy.data_ptr(), st.cuda_stream)
    st.synchronize()
    nn, gur, gz, gxy = n.cpu().numpy(), ur.cpu().numpy(), z.cpu().numpy(), xy.cpu().numpy()
    for b, i in enumerate(idx):
        m = int(nn[b])
        k, d, exy, eur, ez = exp[i]
        assert m == len(k), tag + " batched count"
        assert gxy[b, :m].tobytes() == np.ascontiguousarray(exy, f32).tobytes(), tag + " batched xy"
        assert (T._u32(gur[b, :m]) == T._u32(eur)).all() and (T._u32(gz[b, :m]) == T._u32(ez)).all(), tag + " batched"
        assert (gur[b, m:] == 9).all() and (gz[b, m:] == 9).all(), tag + " batched sentinel"
    frames += nf
    if trial % 10 == 0:
        print(f"{time.time() - t0:6.1f}s trials {trial} frames {frames}", flush=True)

msg = (f"soak_rgbd: {trial} trials, {frames} frames x (one-call + pipelined + batched device), seed {seed}, {time.time() - t0:.0f} s: "
       f"all bit-exact against the restatement on the oracle's keypoints")
print(msg)
if out:
    open(out, "w").write(msg + "\n")
