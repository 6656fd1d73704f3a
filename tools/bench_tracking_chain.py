"""The per-frame projection searches of Tracking on a resident frame (include/orbx.h: orbx_frame) against the host-pointer calls.
Run on the GPU box: python tools/bench_tracking_chain.py [--chain-only | --per-call-only] [--frames N]

1. per call, host-inclusive (direct ctypes calls on prebuilt structs, so neither path pays Python marshalling of its frame): median and
   p99 of SearchByProjection(CurrentFrame, LastFrame) and SearchByProjection(F, vpMapPoints) on _scene(3, 1000, 1000) of
   tests/test_projection.py, uniform and dense, for the host-pointer call, the resident call (frame made once) and the CPU oracle;
2. the chain of one stereo frame at the KITTI shape (1241 x 376, 1000 features), frame by frame: extract_batch_device (L, R) ->
   stereo_match_batch_device -> DeviceFrame.from_extraction -> last-frame search at th, again at 2*th (mvpMapPoints cleared,
   src/Tracking.cc:1065-1072) -> map-point search (:1463).  The points of frame t are made from frame t-1 (read back outside the clock)."""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import __graft_entry__ as ge

pkg = ge.load_pkg()
f32 = np.float32


def stats(ts):
    a = np.array(ts) * 1e6
    return "median %7.1f us  p99 %7.1f us" % (np.median(a), np.percentile(a, 99))


def per_call(reps=200):
    from test_projection import _scene
    from oracle import oracle_py as O
    L = pkg.lib()
    print("== per call, host-inclusive, _scene(3, 1000, 1000), last-frame th 15 / map points th 3 ==")
    for dense in (False, True):
        cur, pts, sf = _scene(3, 1000, 1000, dense=dense)
        p2 = dict(pts); p2["aux"] = (pts["u"] - 5).astype(f32)
        a, ka = pkg.ORBmatcher._frame(cur); b, kb = pkg.ORBmatcher._points(pts); b2, kb2 = pkg.ORBmatcher._points(p2)
        df = pkg.DeviceFrame({k: cur[k] for k in ("x", "y", "octave", "angle", "u_right", "desc", "bounds")})
        occ = np.ascontiguousarray(cur["occupied"], np.uint8)
        out = np.full(a.n, -1, np.int32); n = C.c_int()
        sfp, op, oc = sf.ctypes.data, out.ctypes.data, occ.ctypes.data
        calls = {
            "last  host    ": lambda: L.orbx_search_by_projection_last_frame(0, C.byref(a), C.byref(b), sfp, 8, 15.0, 0, 40.0, 1, op, C.byref(n)),
            "last  resident": lambda: L.orbx_frame_search_by_projection_last_frame(df._h, oc, C.byref(b), sfp, 8, 15.0, 0, 40.0, 1, op, C.byref(n)),
            "points host    ": lambda: L.orbx_search_by_projection_map_points(0, C.byref(a), C.byref(b2), sfp, 8, 3.0, 0.8, op, C.byref(n)),
            "points resident": lambda: L.orbx_frame_search_by_projection_map_points(df._h, oc, C.byref(b2), sfp, 8, 3.0, 0.8, op, C.byref(n)),
        }
        res = {}
        for name, fn in calls.items():
            for _ in range(10):
                assert fn() == 0
            ts = []
            for _ in range(reps):
                t = time.perf_counter(); rc = fn(); ts.append(time.perf_counter() - t)
                assert rc == 0
            res[name] = (out.copy(), n.value)
            print("%-8s %s %s  matches %d" % ("dense" if dense else "uniform", name, stats(ts), n.value))
        assert (res["last  host    "][0] == res["last  resident"][0]).all() and (res["points host    "][0] == res["points resident"][0]).all()
        for name, fn in (("last  oracle  ", lambda: O.search_by_projection_last(cur, pts, sf, 15.0, 0, 40.0, True)),
                         ("points oracle  ", lambda: O.search_by_projection_points(cur, p2, sf, 3.0, 0.8))):
            ts = []
            for _ in range(20):
                t = time.perf_counter(); fn(); ts.append(time.perf_counter() - t)
            print("%-8s %s %s  (CPU, one host thread, incl. ctypes marshalling)" % ("dense" if dense else "uniform", name, stats(ts)))


def chain(nframes):
    import torch
    from tools import synth
    W, H, BF, MIN_Z = 1241, 376, 386.1448, 386.1448 / 718.856
    dev = torch.device("cuda", 0)
    pitch = (W + 63) // 64 * 64
    ex = pkg.ORBextractor(1000, 1.2, 8, 20, 7, device=0, max_size=(W, H), max_batch=2)
    cap = ex.max_keypoints(W, H)
    sf = ex.GetScaleFactors()
    seq = synth.sequence(61, W + 16, H, nframes + 1)
    imgs = []
    for i in range(nframes + 1):   # the right eye sees the scene 16 px further left: a constant disparity
        host = np.zeros((2, H, pitch), np.uint8)
        host[0, :, :W] = seq[i][:, 16:]; host[1, :, :W] = seq[i][:, :W]
        imgs.append(torch.from_numpy(host).to(dev))
    kps = torch.zeros((2, cap, 7), dtype=torch.float32, device=dev)
    desc = torch.zeros((2, cap, 32), dtype=torch.uint8, device=dev)
    nout = torch.zeros(2, dtype=torch.int32, device=dev)
    ur = torch.zeros((1, cap), dtype=torch.float32, device=dev); dp = torch.zeros((1, cap), dtype=torch.float32, device=dev)
    stream = torch.cuda.Stream(device=dev); sp = stream.cuda_stream
    torch.cuda.synchronize()
    mt, ml = pkg.ORBmatcher(0.9, True), pkg.ORBmatcher(0.8, True)
    rng = np.random.Generator(np.random.PCG64(5))
    prev = None
    rows = []
    th = 7.0
    for i in range(nframes + 1):
        t0 = time.perf_counter()
        ex.extract_batch_device(imgs[i].data_ptr(), H * pitch, pitch, 2, W, H, kps.data_ptr(), desc.data_ptr(), cap, nout.data_ptr(), sp)
        pkg.orbx.stereo_match_batch_device(ex, 0, ex, 1, 1, kps.data_ptr(), desc.data_ptr(), nout.data_ptr(), kps[1:].data_ptr(), desc[1:].data_ptr(),
                                           nout[1:].data_ptr(), cap, BF, MIN_Z, ur.data_ptr(), dp.data_ptr(), sp)
        t1 = time.perf_counter()
        f = pkg.DeviceFrame.from_extraction(0, kps.data_ptr(), desc.data_ptr(), nout.data_ptr(), cap, 0, d_u_right=ur.data_ptr(),
                                            bounds=(0.0, 0.0, float(W), float(H)), stream=sp)
        t2 = time.perf_counter()
        if prev is not None:
            m = len(prev["x"])
            pts = dict(u=(prev["x"] + 2.0).astype(f32), v=prev["y"].copy(), aux=np.full(m, 0.1, f32), level=prev["octave"], angle=prev["angle"],
                       view_cos=np.ones(m, f32), desc=prev["desc"], valid=np.ones(m, np.uint8), has_obs=(rng.random(m) < 0.8).astype(np.uint8))
            p2 = dict(pts); p2["aux"] = np.where(prev["u_right"] > 0, prev["u_right"] + 2.0, -1).astype(f32)
            t3 = time.perf_counter()
            g1, n1 = mt.SearchByProjectionLastFrameResident(f, None, pts, sf, th, 0, BF)
            t4 = time.perf_counter()
            g2, n2 = mt.SearchByProjectionLastFrameResident(f, None, pts, sf, 2 * th, 0, BF)
            t5 = time.perf_counter()
            occ = ((g2 >= 0) & (pts["has_obs"][np.maximum(g2, 0)] == 1)).astype(np.uint8)
            t6 = time.perf_counter()
            g3, n3 = ml.SearchByProjectionMapPointsResident(f, occ, p2, sf, 3.0)
            t7 = time.perf_counter()
            rows.append((t1 - t0, t2 - t1, t4 - t3, t5 - t4, t7 - t6, (t2 - t0) + (t7 - t6) + (t5 - t3), f.n, n1, n2, n3))
        prev = f.read()
    r = np.array(rows[2:])   # the first frames carry the lazy allocations
    print("== chain per stereo frame, KITTI 1241x376 @1000, %d frames (host clock, microseconds, median / p99) ==" % len(r))
    for j, name in enumerate(("extract L+R + stereo (enqueue)", "from_extraction (count read = the wait for extraction + stereo)",
                              "last-frame search th", "last-frame search 2*th", "map-point search", "total")):
        print("  %-66s %8.1f  %8.1f" % (name, np.median(r[:, j]) * 1e6, np.percentile(r[:, j], 99) * 1e6))
    print("  features %d, matches th %d, 2*th %d, map points %d (medians)" % tuple(int(np.median(r[:, j])) for j in range(6, 10)))


if __name__ == "__main__":
    nframes = int(sys.argv[sys.argv.index("--frames") + 1]) if "--frames" in sys.argv else 60
    if "--chain-only" not in sys.argv:
        per_call()
    if "--per-call-only" not in sys.argv:
        chain(nframes)
