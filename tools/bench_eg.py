"""Timing of Optimizer::OptimizeEssentialGraph on the device (orbx_optimize_essential_graph), host-inclusive: a clock round the ABI call,
medians of --reps calls, on loops of 100, 500 and 1500 free keyframes (tests/eg_scene.py's generator, fixed scale, so that the call runs
its iterations instead of stalling in Sim3::log's faulty branch; about 3 map points a keyframe); per-kernel device times through
orbx_debug_eg_profile in calls of their own (every launch between two events and waited for; those calls' wall times are not reported).
Reported, not gated.  There is no reference figure: g2o cannot be built here, and nothing in this repository has timed it.
  --out F   the report is also written to F (profiles/r22_eg.txt)"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SIZES = [100, 500, 1500]
NAMES = ["k_eg_setup", "k_eg_edges<true>", "k_eg_rows", "k_eg_reduce", "k_eg_fill", "solve (panels)", "k_eg_update", "k_eg_edges<false>",
         "k_eg_finish", "k_eg_points"]
STEP_LIMIT = 500
p = lambda a: a.ctypes.data_as(C.c_void_p)


def step(index, reps):
    import __graft_entry__ as ge
    import eg_scene as es
    pkg = ge.load_pkg()
    L = pkg.lib()
    F = SIZES[index]
    pr, keep = pkg.orbx._eg_problem(es.make(F, 1, 5100 + F), "bench_eg")
    T = np.zeros((pr.n_kf, 16), np.float32); X = np.zeros((pr.n_points, 3), np.float32)
    rep = pkg.orbx.EgReport()
    opt = pkg.orbx.EgOptions(20)
    call = lambda: L.orbx_optimize_essential_graph(0, C.byref(pr), C.byref(opt), p(T), p(X), None, None, C.byref(rep))
    for _ in range(2):
        if call() != 0:
            raise SystemExit(L.orbx_last_error().decode())
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ts.append(time.perf_counter() - t0)
    dev = 1e3 * float(np.median(ts))
    print(f"loop free {F} (n = {7 * F}, S {8 * (7 * F) ** 2 / 1e6:.0f} MB) edges {pr.n_edges} points {pr.n_points}: {dev:10.3f} ms per call (iterations "
          f"{rep.iterations}, trials {rep.trials}, failed solves {rep.n_solve_failed}, {dev / max(rep.trials, 1):9.3f} ms per trial, chi2 "
          f"{rep.chi2_start:.4g} -> {rep.chi2:.4g})", flush=True)
    ms = np.zeros(10); cnt = np.zeros(10, np.int32)
    L.orbx_debug_eg_profile(1, None, None)
    call()
    L.orbx_debug_eg_profile(0, p(ms), p(cnt))
    for k in range(10):
        if cnt[k]:
            print(f"  kernel {NAMES[k]:18s} launches per call {cnt[k]:4d}   {1e3 * ms[k] / cnt[k]:11.2f} us per launch   {ms[k]:10.3f} ms per call "
                  f"({100 * ms[k] / ms.sum():5.1f} % of the device time)", flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--step", default="")
    a = ap.parse_args()
    if a.step:
        return step(int(a.step), a.reps)
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

    say(f"# Optimizer::OptimizeEssentialGraph on the device, host-inclusive (a clock round the ABI call), medians of {a.reps} calls; device: "
        f"{pkg.orbx.device_identity(0)}")
    say("# there is no reference figure: g2o cannot be built here, and nothing in this repository has timed it")
    for i in range(len(SIZES)):
        cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--step", str(i)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMIT)
        except subprocess.TimeoutExpired:
            say(f"# step {i}: no result within {STEP_LIMIT} s; stopping")
            return 1
        if r.returncode != 0:
            say(f"# step {i}: exit status {r.returncode}; stopping\n{r.stdout}{r.stderr[-600:]}")
            return 1
        say(r.stdout.rstrip())
    return 0


if __name__ == "__main__":
    sys.exit(main())
