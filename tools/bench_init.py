"""Host-inclusive cost of Initializer::Initialize on the device (reference src/Initializer.cc:52-1026) for n in {100, 300, 1000} matches at
200 hypotheses; medians of --reps calls, in microseconds:
  initialize   orbx_mono_init_initialize through ctypes, arguments prepared once (the clock holds the call alone: refusals, Normalize and
               the packing copy, the acos thresholds, one upload, k_mono_hyp + k_mono_reconstruct + k_mono_decide, one download)
  table        orbx_mono_init_hypotheses alone (one launch; the whole table comes down)
  reconstruct  orbx_mono_init_reconstruct alone on the table's winner (two launches)
  mirror       mono_init_initialize of the Python mirror (numpy conversions and result arrays inside the clock)
  adaptor      tests/adapter_init_driver.cc `bench`: the compiled ORB_SLAM2::Initializer with its own work inside the clock -- the
               constructor, the gather, mvMatches12, the draw of mvSets, the one device call, the filling of the outputs
  plain C++    tools/init_baseline.cc: the TABLE alone (not the reconstruction) on one host core without cv::Mat; its bits are compared
               with the device's
  kernels      --trace: the adaptor's bench again under rocprofv3 --kernel-trace --stats, a run of its own whose timings are not
               reported: the three kernels' own average times
Every configuration of every form runs as a child process under its own time limit; a child that fails or runs out of time ends the tool.
Reported, not gated.  The reference's Initializer needs OpenCV, which is not available where this runs, and nothing in the repository has
timed it: no speed-up over the reference is claimed.
Needs an MI355X: python tools/bench_init.py [--out FILE] [--reps 200] [--trace]"""
import argparse
import csv
import ctypes as C
import glob
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = (100, 300, 1000)      # matches; 200 hypotheses each
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


def step(n, reps, baseline_so):
    """one size in this process: the three ABI calls, the mirror and the plain C++ loop on the same job"""
    import numpy as np
    import __graft_entry__ as ge
    import init_model as im
    import init_scene as sc
    pkg = ge.load_pkg()
    ox, L = pkg.orbx, pkg.lib()
    j = dict(sc.job("general", n, 200))
    J, keep, out = ox._mono_init_job(j, "bench")
    P3D, tri = np.zeros((J.n1, 3), np.float32), np.zeros(J.n1, np.uint8)
    res = ox.MonoInitResult(P3D=P3D.ctypes.data, triangulated=tri.ctypes.data)
    init = lambda: L.orbx_mono_init_initialize(0, C.byref(J), C.byref(res))
    table = lambda: L.orbx_mono_init_hypotheses(0, C.byref(J))
    assert init() == 0 and table() == 0, L.orbx_last_error()
    dev = tuple(a.copy() for a in out)
    ch = im.choose(dev)
    best, M, mask = (ch["best_h"], dev[1], dev[2]) if ch["model"] == 1 else (ch["best_f"], dev[4], dev[5])
    Mw, mw = np.ascontiguousarray(M[best]), np.ascontiguousarray(mask[best])
    rec = ox.MonoInitRecon(P3D=P3D.ctypes.data, triangulated=tri.ctypes.data)
    recon = lambda: L.orbx_mono_init_reconstruct(0, C.byref(J), ch["model"], Mw.ctypes.data, mw.ctypes.data, C.byref(rec))
    assert recon() == 0, L.orbx_last_error()
    t_init, t_table, t_rec = median_us(init, reps), median_us(table, reps), median_us(recon, reps)
    t_mirror = median_us(lambda: pkg.mono_init_initialize(j), reps)
    B = C.CDLL(baseline_so)
    B.mono_init_table_loop.argtypes = [C.POINTER(ox.MonoInitJob)]
    base = lambda: B.mono_init_table_loop(C.byref(J))
    assert base() == 0
    same = all(a.tobytes() == b.tobytes() for a, b in zip(out, dev))
    t_base = median_us(base, max(5, reps // 20))
    faster = "the device call" if t_table < t_base else "the plain loop"
    print(f"{n} matches of {J.n1} / {J.n2} keypoints x 200 hypotheses (model {res.model}, ok {res.ok}, n_good {list(res.n_good)}):\n"
          f"  initialize (orbx_mono_init_initialize)     {t_init:9.1f}\n"
          f"  table alone (orbx_mono_init_hypotheses)    {t_table:9.1f}\n"
          f"  reconstruct alone (the table's winner)     {t_rec:9.1f}\n"
          f"  Python mirror (mono_init_initialize)       {t_mirror:9.1f}\n"
          f"  plain C++ loop, the table on one host core {t_base:9.1f}   (scores, matrices and masks equal the device's: {same}; faster: {faster})",
          flush=True)
    L.orbx_thread_release()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--step", nargs=2, type=str, default=None, help=argparse.SUPPRESS)   # matches baseline.so: a child
    a = ap.parse_args()
    if a.step:
        step(int(a.step[0]), a.reps, a.step[1])
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

    say(f"# Initializer::Initialize on the device, host-inclusive (a clock round the call), medians of {a.reps} calls in microseconds; "
        f"device: {pkg.orbx.device_identity(0)}")
    say("# no reference figure exists: the reference's Initializer needs OpenCV and the repository has never timed it")
    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "libinit_baseline.so")
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++11", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tools", "init_baseline.cc"), "-o", so])
        import test_init_adapter as ta
        exe = ta.build_driver(tmp)
        for n in SHAPES:
            cmds = [[sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--step", str(n), so], [exe, "bench", str(n), str(a.reps)]]
            for cmd in cmds:
                try:
                    r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMIT)
                except subprocess.TimeoutExpired:
                    say(f"# {' '.join(cmd[-3:])}: no result within {STEP_LIMIT} s; stopping")
                    return 1
                if r.returncode != 0:
                    say(f"# {' '.join(cmd[-3:])}: exit status {r.returncode}; stopping\n{r.stdout}{r.stderr}")
                    return 1
                say(("  " if cmd[0] == exe else "") + r.stdout.rstrip())
            if a.trace:
                out = os.path.join(tmp, f"trace{n}")
                try:
                    run = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", exe, "bench", str(n), "50"],
                                         capture_output=True, text=True, timeout=STEP_LIMIT)
                except subprocess.TimeoutExpired:
                    say(f"# kernel trace at {n}: no result within {STEP_LIMIT} s; stopping")
                    return 1
                if run.returncode != 0:
                    say(f"# kernel trace at {n}: exit status {run.returncode}; stopping\n{run.stderr[-400:]}")
                    return 1
                found = False
                for path in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
                    for row in csv.DictReader(open(path)):
                        if "k_mono_" in row.get("Name", ""):
                            name = re.search(r"k_mono_\w+", row["Name"]).group(0)
                            say(f"  kernel {name:20s} calls {row.get('Calls')}   average {float(row.get('AverageNs', 'nan')) / 1000.0:7.2f} us   "
                                f"min {float(row.get('MinNs', 'nan')) / 1000.0:7.2f}   max {float(row.get('MaxNs', 'nan')) / 1000.0:7.2f}   (under the profiler)")
                            found = True
                if not found:
                    say("  kernel trace: no stats file found: " + run.stderr.strip()[-300:])
    return 0


if __name__ == "__main__":
    sys.exit(main())
