"""Host-inclusive cost of Optimizer::PoseOptimization on the device (reference src/Optimizer.cc:286-513), through the Python mirror's ctypes
calls prepared once (the clock holds the ABI call alone):
  host      orbx_pose_optimize: observations from host pointers, one upload, one launch, one download
  resident  orbx_frame_pose_optimize: frame and map points resident, n int32 slots and the pose up
  batch     orbx_pose_optimize_batch with 8 and 32 equal jobs, reported PER JOB
at 100, 300 and 1000 correspondences with 20 % gross outliers; medians of --reps calls.  The kernel's own time is not in this file: the
resident form's single call is the kernel plus one small upload, one launch and one download.
Reported, not gated.  What this replaces -- g2o's Levenberg solver on a host core -- cannot be built here (it needs Eigen) and nothing in the
repository has timed it: there is no figure to set these against, and none is claimed.  The one comparison inside this file is batch per
job against the single call, both new code.
Run on the GPU box: python tools/bench_pose_opt.py [--out FILE] [--reps 200]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge                    # noqa: E402
import pose_scene as ps                         # noqa: E402

SIZES = (100, 300, 1000)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    pkg = ge.build()
    ox, L = pkg.orbx, pkg.lib()
    p = lambda arr: arr.ctypes.data_as(C.c_void_p)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# PoseOptimization on the device, host-inclusive (time.perf_counter round the ABI call), medians of {a.reps} calls in microseconds; "
        f"device: {ox.device_identity(0)}")
    say("# no reference figure exists: g2o cannot be built here (no Eigen) and the repository has never timed it")
    for n in SIZES:
        sc = ps.scene(900 + n, n, "mixed", outlier_frac=0.2)
        po, keep = ox._pose_obs(sc["obs"], "bench")
        cam = np.ascontiguousarray(sc["cam"], f32); T = np.ascontiguousarray(sc["Tcw"], f32).reshape(-1)
        out = np.zeros(16, f32); fl = np.zeros(po.n, np.uint8); ni = C.c_int(); rep = ox.PoseReport()
        host = lambda: L.orbx_pose_optimize(0, C.byref(po), p(cam), p(T), p(out), p(fl), C.byref(ni), C.byref(rep))
        assert host() == 0
        t_host = median_us(host, a.reps)
        head = f"{n} correspondences of {po.n} features: inliers {ni.value}, n_bad {list(rep.n_bad)}, iterations {list(rep.iterations)}"
        nfeat = po.n
        rng = np.random.Generator(np.random.PCG64(n))
        frame = dict(x=sc["obs"]["x"], y=sc["obs"]["y"], octave=sc["octave"], angle=np.zeros(nfeat, f32), u_right=sc["obs"]["u_right"],
                     desc=rng.integers(0, 256, (nfeat, 32), dtype=np.uint8), bounds=(0.0, 0.0, float(ps.W), float(ps.H)))
        df = pkg.DeviceFrame(frame)
        has = sc["obs"]["has_point"].astype(bool)
        slot = np.full(nfeat, -1, np.int32); slot[has] = rng.permutation(4096)[:n]
        geom = np.ones((n, 8), f32); geom[:, :3] = sc["obs"]["Xw"][has]
        mp = pkg.MapPoints(4096)
        mp.set(slot[has], geom, np.zeros((n, 32), np.uint8))
        isig = ps.INV_SIGMA2
        out2 = np.zeros(16, f32); fl2 = np.zeros(nfeat, np.uint8)
        res = lambda: L.orbx_frame_pose_optimize(df._h, mp._h, p(slot), p(isig), len(isig), p(cam), p(T), p(out2), p(fl2), C.byref(ni), None)
        assert res() == 0 and out2.tobytes() == out.tobytes()
        t_res = median_us(res, a.reps)
        t_batch = {}
        for nb in (8, 32):
            jobs = (ox.PoseJob * nb)()
            outs = [np.zeros(16, f32) for _ in range(nb)]; fls = [np.zeros(nfeat, np.uint8) for _ in range(nb)]
            for j in range(nb):
                jobs[j].obs = C.pointer(po); jobs[j].cam = p(cam); jobs[j].Tcw = p(T); jobs[j].Tcw_out = p(outs[j]); jobs[j].outlier = p(fls[j])
            bat = lambda: L.orbx_pose_optimize_batch(0, jobs, nb)
            assert bat() == 0 and outs[nb - 1].tobytes() == out.tobytes()
            t_batch[nb] = median_us(bat, a.reps) / nb
        say(head)
        say(f"  host pointers, single call          {t_host:8.1f}")
        say(f"  resident frame + map points         {t_res:8.1f}")
        say(f"  batch of  8, per job                {t_batch[8]:8.1f}   ({t_host / t_batch[8]:.2f}x the single call's rate)")
        say(f"  batch of 32, per job                {t_batch[32]:8.1f}   ({t_host / t_batch[32]:.2f}x the single call's rate)")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
