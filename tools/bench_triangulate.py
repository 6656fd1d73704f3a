"""Host-inclusive cost of the triangulation half of LocalMapping::CreateNewMapPoints on the device (reference src/LocalMapping.cc:327-511),
through ctypes calls prepared once (the clock holds the ABI call alone):
  host      orbx_triangulate_pairs: every keyframe's arrays from host pointers, one upload, three launches, one download
  resident  orbx_frame_triangulate: keyframes resident, the views and the pair lists up
  plain C++ tools/tri_baseline.cc: the same arithmetic on one host core without cv::Mat, neighbour by neighbour -- a LOWER BOUND on the
            reference's loop body (no cv::Mat temporaries, no cv::SVD, no allocation), not the reference
for 10 and 20 neighbours of about 200 pairs each, keyframes of 2000 features, 30 % stereo features; medians of --reps calls.
Reported, not gated.  The reference's own loop needs OpenCV, which is not available where this runs, and nothing in the repository has
timed it: no speed-up over the reference is claimed.
Needs an MI355X: python tools/bench_triangulate.py [--out FILE] [--reps 200]"""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge                    # noqa: E402
import triangulate_scene as ts                  # noqa: E402

f32 = np.float32


def median_us(fn, reps):
    for _ in range(5):
        fn()
    t = []
    for _ in range(reps):
        a = time.perf_counter()
        fn()
        t.append((time.perf_counter() - a) * 1e6)
    return statistics.median(t)


def baseline_lib(tmp):
    so = os.path.join(tmp, "libtri_baseline.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++11", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tools", "tri_baseline.cc"), "-o", so])
    return C.CDLL(so)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    pkg = ge.build()
    ox, L = pkg.orbx, pkg.lib()
    p = ox._p
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# CreateNewMapPoints' triangulation on the device, host-inclusive (time.perf_counter round the call), medians of {a.reps} calls in "
        f"microseconds; device: {ox.device_identity(0)}")
    say("# no reference figure exists: the reference's loop needs OpenCV and the repository has never timed it")
    ts.N1 = 2000
    with tempfile.TemporaryDirectory() as tmp:
        B = baseline_lib(tmp)
        for n2 in (10, 20):
            s = ts.make_scene(1400 + n2, (200 - n2 // 10,) * n2, stereo1=0.3, stereo2=0.3, close=(3,), name=f"bench{n2}")
            f1, keep1 = ox._tri_feats(s["k1"], "bench")
            fs = [ox._tri_feats(k, "bench") for k in s["k2s"]]
            ptrs = (C.POINTER(ox.TriFeats) * n2)(*[C.pointer(f[0]) for f in fs])
            views = (ox.TriView * n2)(*[ox._tri_view(v, "bench") for v in s["v2s"]])
            v1 = ox._tri_view(s["v1"], "bench")
            cap = s["cap"]
            st = np.zeros((n2, cap), np.uint8); x = np.zeros((n2, cap, 3), f32); nn = C.c_int()
            tail = (n2, p(s["pairs"]), cap, p(s["npairs"]), p(s["sf"]), p(s["sigma2"]), len(s["sf"]), float(s["ratio_factor"]))
            host = lambda: L.orbx_triangulate_pairs(0, C.byref(f1), C.byref(v1), ptrs, views, *tail, p(st), p(x), C.byref(nn))
            assert host() == 0
            t_host = median_us(host, a.reps)
            frames = []
            for k in [s["k1"]] + s["k2s"]:
                n = len(k["x"])
                df = pkg.DeviceFrame(dict(x=k["x"], y=k["y"], octave=k["octave"], angle=np.zeros(n, f32), u_right=k["u_right"],
                                          desc=np.zeros((n, 32), np.uint8), bounds=(-2000.0, -2000.0, 3000.0, 3000.0)))
                pkg.frame_set_depth(df, k["depth"])
                frames.append(df)
            hs = (C.c_void_p * n2)(*[f._h for f in frames[1:]])
            st2 = np.zeros_like(st); x2 = np.zeros_like(x); nn2 = C.c_int()
            res = lambda: L.orbx_frame_triangulate(frames[0]._h, C.byref(v1), hs, views, *tail, p(st2), p(x2), C.byref(nn2))
            assert res() == 0 and st2.tobytes() == st.tobytes() and x2.tobytes() == x.tobytes() and nn2.value == nn.value
            t_res = median_us(res, a.reps)
            st3 = np.zeros_like(st); x3 = np.zeros_like(x)
            B.tri_loop.argtypes = [C.POINTER(ox.TriFeats), C.POINTER(ox.TriView), C.POINTER(C.POINTER(ox.TriFeats)), C.POINTER(ox.TriView), C.c_int,
                                   C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]
            base = lambda: B.tri_loop(C.byref(f1), C.byref(v1), ptrs, views, n2, p(s["pairs"]), cap, p(s["npairs"]), p(s["sf"]), p(s["sigma2"]),
                                      float(s["ratio_factor"]), p(st3), p(x3))
            n_base = base()
            seen = st3 != 255                      # the pairs the sequential loop reaches (cap == every list's length here)
            # a pair the loop skips is superseded on the device if it would have been created, and rejected otherwise
            same = bool((st[~seen] >= 16).all() and (st[seen] < 32).all() and (st3[seen] == st[seen]).all() and
                        x3[seen].tobytes() == x[seen].tobytes() and n_base == nn.value)
            t_base = median_us(base, a.reps)
            total = int(s["npairs"].sum())
            say(f"{n2} neighbours, {total} pairs, keyframes of {ts.N1} features: created {nn.value}, superseded {int((st >= 32).sum())}, "
                f"rejected {total - nn.value - int((st >= 32).sum())}")
            say(f"  host pointers (orbx_triangulate_pairs)     {t_host:8.1f}")
            say(f"  resident frames (orbx_frame_triangulate)   {t_res:8.1f}")
            say(f"  plain C++ loop on one host core            {t_base:8.1f}   (created {n_base}; statuses and x3d bits equal the device's: {same}; "
                f"it tests {int(seen.sum())} pairs, the superseded ones never reach the reference's loop body)")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
