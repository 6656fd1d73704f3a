"""RGB-D measurements -> profiles/r05_rgbd.txt.  Run on the GPU box: python tools/bench_rgbd.py [out] [--batched-only]
  1. one frame, host-inclusive p50 / p99 at 640 x 480 with uint16 depth (TUM1): orbx_extract_rgbd against orbx_extract alone and against the
     path an RGB-D user has without it (orbx_extract + orbx_undistort_keypoints + ComputeStereoFromRGBD on the host, here a vectorised numpy
     pass over the keypoints -- the reference's loop of ~1000 reads);
  2. a camera stream: examples/rgbd_stream (plain C client of the pipelined form), grey and colour, both depth transports, 1 and 4 frames in flight;
  3. batched throughput, B = 256: orbx_extract_batch_device alone against + orbx_rgbd_depth_batch_device (torch events, 20 steps).
--batched-only runs 3 alone (the rocprofv3 pass that gives k_rgbd_depth's average)."""
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import __graft_entry__ as ge  # noqa: E402
from tools import synth  # noqa: E402

FIX = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_settings_rgbd.json")))["TUM1 rgbd"]
W, H, NF = int(FIX["Camera.width"]), int(FIX["Camera.height"]), int(FIX["ORBextractor.nFeatures"])
f32 = np.float32


def pct(a, q):
    return float(np.percentile(np.asarray(a) * 1e6, q))


def single_frame(pkg, lines, reps=300):
    from test_rgbd import _depth_u16, restate
    ex = pkg.ORBextractor(NF, 1.2, 8, 20, 7, device=0, max_size=(W, H), max_batch=2)
    p = pkg.RGBDParams.from_settings(FIX)
    img = synth.image(5, W, H)
    raw = _depth_u16(5)
    for _ in range(20):
        ex.extract_rgbd(img, raw, p); ex(img)
    t_one, t_mono, t_old = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter(); ex.extract_rgbd(img, raw, p); t_one.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); ex(img); t_mono.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        k, d = ex(img)
        xy = pkg.UndistortKeyPoints(np.stack([k["x"], k["y"]], 1), p.fx, p.fy, p.cx, p.cy, p.dist_coef)
        restate(k["x"], k["y"], xy[:, 0], raw, p.depth_scale, p.bf)
        t_old.append(time.perf_counter() - t0)
    lines.append(f"## 1. one frame, host-inclusive (Python ctypes caller), 640x480 @ {NF}, uint16 depth, TUM1, {reps} frames each")
    for name, t in (("orbx_extract_rgbd (one call)", t_one), ("orbx_extract alone", t_mono),
                    ("orbx_extract + orbx_undistort_keypoints + host lookup (numpy)", t_old)):
        lines.append(f"{name:66s} p50 {pct(t, 50):8.1f} us   p99 {pct(t, 99):8.1f} us")
    lines.append(f"one call - orbx_extract alone (p50): {pct(t_one, 50) - pct(t_mono, 50):.1f} us")
    lines.append("")


def stream(lines, frames=2000):
    exe = os.path.join(tempfile.mkdtemp(), "rgbd_stream")
    lib = os.path.join(ROOT, "orb-slam2_amd")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "rgbd_stream.c"),
                           "-L", lib, "-lorbx", "-Wl,-rpath," + lib, "-o", exe])
    lines.append(f"## 2. camera stream: examples/rgbd_stream, one handle, {frames} frames per run, pinned frame buffers, uint16 depth")
    for ch in (1, 3):
        for gather in ("0", "1"):
            env = dict(os.environ, ORBX_PIPE_RGBD_GATHER=gather)
            out = subprocess.run([exe, "--frames", str(frames), "--channels", str(ch)], env=env, capture_output=True, text=True, timeout=300)
            if out.returncode != 0:
                raise RuntimeError(out.stderr)
            j = json.loads(out.stdout.strip().splitlines()[-1])
            for k in ("in_flight_1", "in_flight_4"):
                r = j[k]
                lines.append(f"channels {ch}  transport {j['depth_transport']:6s}  {k:12s}  {r['frames_per_s']:9.1f} frames/s   "
                             f"p50 {r['latency_us_p50']:7.1f} us   p99 {r['latency_us_p99']:7.1f} us")
    lines.append("")


def batched(pkg, lines, B=256, steps=20):
    import torch
    from test_rgbd import _depth_u16
    dev = torch.device("cuda", 0)
    ex = pkg.ORBextractor(NF, 1.2, 8, 20, 7, device=0, max_size=(W, H), max_batch=B)
    p = pkg.RGBDParams.from_settings(FIX)
    pitch = (W + 63) // 64 * 64
    host = np.zeros((B, H, pitch), np.uint8)
    for i in range(B):
        host[i, :, :W] = synth.image(1000 + i % 16, W, H)
    dep = np.stack([_depth_u16(2000 + i % 16) for i in range(B)])
    t_img = torch.from_numpy(host).to(dev); t_dep = torch.from_numpy(dep).to(dev)
    cap = ex.max_keypoints(W, H)
    kps = torch.zeros((B, cap, 7), dtype=torch.float32, device=dev)
    desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device=dev)
    n = torch.zeros(B, dtype=torch.int32, device=dev)
    ur = torch.zeros((B, cap), dtype=torch.float32, device=dev); z = torch.zeros_like(ur); xy = torch.zeros((B, cap, 2), dtype=torch.float32, device=dev)
    st = torch.cuda.Stream(device=dev)
    sp = st.cuda_stream

    def step(with_depth):
        ex.extract_batch_device(t_img.data_ptr(), H * pitch, pitch, B, W, H, kps.data_ptr(), desc.data_ptr(), cap, n.data_ptr(), sp)
        if with_depth:
            pkg.rgbd_depth_batch_device(0, kps.data_ptr(), n.data_ptr(), cap, B, t_dep.data_ptr(), H * W * 2, W * 2, W, H, p, pkg.DEPTH_U16,
                                        ur.data_ptr(), z.data_ptr(), xy.data_ptr(), sp)

    res = {}
    for with_depth in (False, True, False, True):
        for _ in range(3):
            step(with_depth)
        st.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(steps):
            step(with_depth)
        e1.record(st)
        e1.synchronize()
        res[with_depth] = e0.elapsed_time(e1) / steps * 1e3      # us per step (the second pass of each kind is kept)
    # the depth kernel alone, on the last extraction's outputs
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(steps):
        pkg.rgbd_depth_batch_device(0, kps.data_ptr(), n.data_ptr(), cap, B, t_dep.data_ptr(), H * W * 2, W * 2, W, H, p, pkg.DEPTH_U16,
                                    ur.data_ptr(), z.data_ptr(), xy.data_ptr(), sp)
    e1.record(st)
    e1.synchronize()
    alone = e0.elapsed_time(e1) / steps * 1e3
    lines.append(f"## 3. batched, B = {B} at {W}x{H} @ {NF}, device-resident images and uint16 depth, {steps} steps (torch events)")
    lines.append(f"orbx_extract_batch_device alone                      {res[False]:9.1f} us per step   {B / res[False] * 1e6:10.0f} frames/s")
    lines.append(f"  + orbx_rgbd_depth_batch_device                     {res[True]:9.1f} us per step   {B / res[True] * 1e6:10.0f} frames/s")
    lines.append(f"orbx_rgbd_depth_batch_device alone (back to back)    {alone:9.1f} us per launch  ({100 * alone / res[False]:.2f} % of the extraction step)")
    lines.append("")


def main():
    pkg = ge.build()
    out = next((a for a in sys.argv[1:] if not a.startswith("--")), os.path.join(ROOT, "profiles", "r05_rgbd.txt"))
    lines = []
    if "--batched-only" in sys.argv:
        batched(pkg, lines)
        print("\n".join(lines))
        return
    lines.append("# RGB-D front end on one MI355X (tools/bench_rgbd.py)")
    lines.append(f"device: {pkg.orbx.device_identity(0)}")
    lines.append("")
    single_frame(pkg, lines)
    stream(lines)
    batched(pkg, lines)
    txt = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(out), exist_ok=True)
    open(out, "w").write(txt)
    print(txt)


if __name__ == "__main__":
    main()
