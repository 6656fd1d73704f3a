"""Host-inclusive cost of Fuse's search half against a keyframe (reference src/ORBmatcher.cc:873-1038), three ways:
  host-pointer   orbx_window_best: the keyframe's arrays staged and uploaded, the grid built, lists + resolve kernels, per call
  resident       orbx_frame_window_best on an orbx_frame made once: the points up, one fused kernel, the results down
  batch          orbx_frame_window_best_batch, 20 (keyframe, points) jobs in one upload / launch / download, reported per target
beside the CPU oracle's window_best on one host core, and -- through the compiled adaptor (tests/adapter_kfframe_driver.cc `bench`) -- the
first loop of LocalMapping::SearchInNeighbors as 20 Fuse calls (host-pointer, resident) against one orbx_adapter::FuseBatch, with the
adaptor's projection, staging and map surgery inside the clock.
Scenes: tests/test_projection._scene, uniform and dense, 1000 features x 1000 points, th 3, chi2 gate, TH_LOW.  The C entry points are
called with prebuilt argument structs, so the clock holds the call and nothing of Python's array handling; host-pointer and resident calls
alternate inside one loop.  Exit status 1 unless the resident median is below the host-pointer median on both scenes.
Run on the GPU box: python tools/bench_kf_fuse.py [--out FILE] [--reps 200]"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np                     # noqa: E402
import __graft_entry__ as ge           # noqa: E402
from oracle import oracle_py as O      # noqa: E402
import test_projection as TP           # noqa: E402

f32 = np.float32
FR = ("x", "y", "octave", "angle", "u_right", "desc", "bounds")
TARGETS = 20


def pct(v, q):
    return float(np.percentile(np.asarray(v), q))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    pkg = ge.build()
    L = pkg.lib()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# Fuse search half, host-inclusive, medians of {a.reps} calls in microseconds; device: {pkg.orbx.device_identity(0)}")
    ok = True
    for name, dense in (("uniform", False), ("dense", True)):
        scenes = []
        for t in range(TARGETS):
            cur, pts, sf = TP._scene(800 + t + (100 if dense else 0), 1000, 1000, dense=dense)
            p2 = dict(pts); p2["aux"] = (pts["u"] - 8).astype(f32)
            scenes.append((cur, p2))
        inv = (1.0 / (sf * sf)).astype(f32)
        cur, p2 = scenes[0]
        ff, keep_f = pkg.ORBmatcher._frame(cur)
        pp, keep_p = pkg.ORBmatcher._points(p2)
        frames = [pkg.DeviceFrame({k: c[k] for k in FR}) for c, _ in scenes]
        n = pp.n
        bi_h = np.full(n, -1, np.int32); bi_r = np.full(n, -1, np.int32); nf_h = C.c_int(); nf_r = C.c_int()

        def host():
            return L.orbx_window_best(0, C.byref(ff), C.byref(pp), sf.ctypes.data, inv.ctypes.data, 8, 3.0, 1, 50, bi_h.ctypes.data, None, C.byref(nf_h))

        def resident():
            return L.orbx_frame_window_best(frames[0]._h, C.byref(pp), sf.ctypes.data, inv.ctypes.data, 8, 3.0, 1, 50, bi_r.ctypes.data, None, C.byref(nf_r))

        # the batch: 20 keyframes, each with its own projected points
        jobs = (pkg.orbx.WindowJob * TARGETS)()
        keep = []
        outs = []
        for t, (c, p) in enumerate(scenes):
            q, kq = pkg.ORBmatcher._points(p)
            b = np.full(q.n, -1, np.int32)
            keep.append((q, kq)); outs.append(b)
            w = jobs[t]
            w.kf = frames[t]._h.value; w.pts = C.pointer(q); w.scale_factors = sf.ctypes.data; w.inv_sigma2 = inv.ctypes.data
            w.nlevels = 8; w.th = 3.0; w.chi2 = 1; w.max_dist = 50; w.best_idx = b.ctypes.data; w.best_dist = None

        def batch():
            return L.orbx_frame_window_best_batch(jobs, TARGETS)

        for _ in range(20):                                   # warm-up of every form
            assert host() == 0 and resident() == 0 and batch() == 0
        ebi, ebd, en = O.window_best(cur, p2, sf, inv, 3.0, 1, 50)
        assert nf_h.value == nf_r.value == en and (bi_h == ebi).all() and (bi_r == ebi).all() and (outs[0] == ebi).all(), "results differ from the oracle"
        for t in (7, 19):
            e7 = O.window_best(scenes[t][0], scenes[t][1], sf, inv, 3.0, 1, 50)[0]
            assert (outs[t] == e7).all(), "batch job differs from the oracle"
        th, tr, tb, to = [], [], [], []
        clk = time.perf_counter
        for _ in range(a.reps):                               # the three forms alternate: what disturbs one disturbs all
            t0 = clk(); host(); t1 = clk(); resident(); t2 = clk(); batch(); t3 = clk()
            th.append((t1 - t0) * 1e6); tr.append((t2 - t1) * 1e6); tb.append((t3 - t2) * 1e6 / TARGETS)
        for _ in range(max(a.reps // 4, 10)):
            t0 = clk(); O.window_best(cur, p2, sf, inv, 3.0, 1, 50); to.append((clk() - t0) * 1e6)
        say(f"{name}: 1000 features x 1000 points, found {en}")
        say(f"  host-pointer orbx_window_best        median {pct(th, 50):8.1f}   p10 {pct(th, 10):8.1f}   p90 {pct(th, 90):8.1f}   (its own spread)")
        say(f"  resident orbx_frame_window_best      median {pct(tr, 50):8.1f}   p10 {pct(tr, 10):8.1f}   p90 {pct(tr, 90):8.1f}")
        say(f"  batch of {TARGETS} targets, per target       median {pct(tb, 50):8.1f}   p10 {pct(tb, 10):8.1f}   p90 {pct(tb, 90):8.1f}   (one call: {pct(tb, 50) * TARGETS:.1f})")
        say(f"  CPU oracle window_best, one core     median {pct(to, 50):8.1f}")
        good = pct(tr, 50) < pct(th, 50)
        say(f"  resident below host-pointer: {'yes' if good else 'NO'} ({pct(th, 50) / pct(tr, 50):.2f}x)")
        ok = ok and good
    # the compiled adaptor: the loop of 20 Fuse calls against one FuseBatch, 20 targets x 1000 points x 1200 features
    ad = os.path.join(ROOT, "adapter")
    srcs = [os.path.join(ad, f) for f in ("ORBextractor.cc", "Frame_stereo.cc", "ORBmatcher_bow.cc", "ORBmatcher_proj.cc", "ORBmatcher_fuse.cc", "Frame_bow.cc",
                                          "MapPoint_distinctive.cc", "ORBmatcher_batch.cc")]
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "adapter_kfframe_driver")
        subprocess.check_call(["g++", "-std=c++11", "-O2", "-I", ad, "-I", os.path.join(ROOT, "tests", "cvstub"), "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "adapter_kfframe_driver.cc")] + srcs +
                              ["-L", os.path.join(ROOT, "orb-slam2_amd"), "-lorbx", "-lpthread", "-Wl,-rpath," + os.path.join(ROOT, "orb-slam2_amd"), "-o", exe])
        run = subprocess.run([exe, "bench", "30"], capture_output=True, text=True, timeout=600)
    say("adaptor (compiled, projection + staging + surgery inside the clock), 20 targets x 1000 points, 1200 features per keyframe, medians of 30:")
    for line in run.stdout.strip().splitlines():
        say("  " + line)
    if run.returncode != 0:
        say("  adaptor bench FAILED: " + run.stderr.strip())
        ok = False
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
