"""Host-inclusive cost of PnPsolver's EPnP RANSAC hypotheses on the device (reference src/PnPsolver.cc:193-350) for the shapes
1 candidate x 35 rows x 100 correspondences, 10 x 35 x 100 and 10 x 300 x 1000; medians of --reps calls, in microseconds:
  ABI call  orbx_pnp_hypotheses_batch through ctypes, arguments prepared once (the clock holds the call alone: refusals, staging, one
            upload, k_pnp, one download, delivery)
  mirror    pnp_hypotheses_batch of the Python mirror (numpy conversions and result arrays inside the clock)
  adaptor   tests/adapter_pnp_driver.cc `bench`: the compiled ORB_SLAM2::PnPsolver with its own work inside the clock -- the gather of the
            constructors, SetRansacParameters, the draw, PnPsolverBatch's one device call, and one iterate(5) per candidate
  plain C++ tools/pnp_baseline.cc: the same arithmetic on one host core without cv::Mat, every row of the table evaluated and every
            qualifying row refined, as the device does; its bits are compared with the device's
Every configuration of every form runs as a child process under its own time limit; a child that fails or runs out of time ends the tool.
Reported, not gated.  The reference's solver needs OpenCV, which is not available where this runs, and nothing in the repository has
timed it: no speed-up over the reference is claimed.  The kernel's own time is not measured here (a profiler run of its own gives it).
Needs an MI355X: python tools/bench_pnp.py [--out FILE] [--reps 200]"""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = ((1, 35, 100), (10, 35, 100), (10, 300, 1000))      # candidates, rows, correspondences
STEP_LIMIT = 240    # seconds per child


def median_us(fn, reps):
    for _ in range(5):
        fn()
    t = []
    for _ in range(reps):
        a = time.perf_counter()
        fn()
        t.append((time.perf_counter() - a) * 1e6)
    return statistics.median(t)


def step(ncand, rows, n, reps, baseline_so):
    """one configuration in this process: the ABI call, the mirror and the plain C++ loop on the same jobs"""
    import __graft_entry__ as ge
    import pnp_scene as sc
    pkg = ge.load_pkg()
    ox, L = pkg.orbx, pkg.lib()
    jobs = [dict(sc.job(900 + c, n, rows, n // 2)) for c in range(ncand)]
    arr = (ox.PnpJob * ncand)()
    keep = []
    for c, j in enumerate(jobs):
        J, k, out = ox._pnp_job(j, "bench")
        arr[c] = J
        keep.append((k, out))
    call = lambda: L.orbx_pnp_hypotheses_batch(0, arr, ncand)
    assert call() == 0, L.orbx_last_error()
    dev = [tuple(a.copy() for a in k[1]) for k in keep]
    t_abi = median_us(call, reps)
    t_mirror = median_us(lambda: pkg.pnp_hypotheses_batch(jobs), reps)
    B = C.CDLL(baseline_so)
    B.pnp_loop.argtypes = [C.POINTER(ox.PnpJob), C.c_int]
    base = lambda: B.pnp_loop(arr, ncand)
    base()
    same = all(a.tobytes() == b.tobytes() for k, d in zip(keep, dev) for a, b in zip(k[1], d))
    t_base = median_us(base, max(5, reps // 20))
    refined = sum(int((d[3] >= 0).sum()) for d in dev)
    best = [int(d[3].max()) for d in dev]
    faster = "the device call" if t_abi < t_base else "the plain loop"
    print(f"{ncand} candidates x {rows} rows x {n} correspondences ({refined} rows refined; best refined counts {best}):\n"
          f"  ABI call (orbx_pnp_hypotheses_batch)       {t_abi:9.1f}\n"
          f"  Python mirror (pnp_hypotheses_batch)       {t_mirror:9.1f}\n"
          f"  plain C++ loop on one host core            {t_base:9.1f}   (counts, masks and pose bits equal the device's: {same}; faster: {faster})",
          flush=True)
    L.orbx_thread_release()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--step", nargs=4, type=str, default=None, help=argparse.SUPPRESS)   # candidates rows correspondences baseline.so: a child
    a = ap.parse_args()
    if a.step:
        step(int(a.step[0]), int(a.step[1]), int(a.step[2]), a.reps, a.step[3])
        return 0
    import __graft_entry__ as ge
    pkg = ge.build()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:                                   # kept up to date: a run that stops early leaves what it measured
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    say(f"# PnPsolver's hypotheses on the device, host-inclusive (a clock round the call), medians of {a.reps} calls in microseconds; "
        f"device: {pkg.orbx.device_identity(0)}")
    say("# no reference figure exists: the reference's solver needs OpenCV and the repository has never timed it")
    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "libpnp_baseline.so")
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++11", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tools", "pnp_baseline.cc"), "-o", so])
        import test_pnp_adapter as ta
        exe = ta.build_driver(tmp)
        for ncand, rows, n in SHAPES:
            for cmd in ([sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--step", str(ncand), str(rows), str(n), so],
                        [exe, "bench", str(ncand), str(n), str(rows), str(a.reps)]):
                try:
                    r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMIT)
                except subprocess.TimeoutExpired:
                    say(f"# {' '.join(cmd[-5:])}: no result within {STEP_LIMIT} s; stopping")
                    return 1
                if r.returncode != 0:
                    say(f"# {' '.join(cmd[-5:])}: exit status {r.returncode}; stopping\n{r.stdout}{r.stderr}")
                    return 1
                say(("  " if cmd[0] == exe else "") + r.stdout.rstrip())
    return 0


if __name__ == "__main__":
    sys.exit(main())
