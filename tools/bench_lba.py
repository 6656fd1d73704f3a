"""Optimizer::LocalBundleAdjustment on the device (orbx_local_bundle_adjustment), host-inclusive: a clock round the ABI call, medians of
--reps calls, for windows of (free, fixed, points, edges) about (10, 10, 1 000, 5 k), (30, 30, 3 000, 20 k), (100, 100, 8 000, 60 k) made
by tests/lba_scene.py.  Next to it the same problem through tools/lba_host_loop.cc, a plain C++ dense-Schur restatement on one host
core, built here: a LOWER BOUND for a host solver of this structure and not the reference -- g2o cannot be built here, nobody has measured
either side against it, nothing is gated on these times and no speed-up over g2o is claimed.
Per shape it then runs five more calls under orbx_debug_lba_profile (every launch between two events and waited for; those calls' wall
times are not reported) and prints each kernel's device time per launch and per damping trial.
  --out F   the report is also written to F (profiles/r20_lba.txt)"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SHAPES = [(10, 10, 1000, 8), (30, 30, 3000, 11), (100, 100, 8000, 13)]      # free, fixed, points, the most views of a point
STEP_LIMIT = 400


def step(index, reps, so):
    """one shape in a process of its own: the device call and the host loop on the same problem"""
    import __graft_entry__ as ge
    import lba_scene as ls
    pkg = ge.load_pkg()
    free, fixed, points, views = SHAPES[index]
    sc = ls.scene(31 + index, free, fixed, points, "mixed", max_views=views)
    pr, keep = pkg.orbx._lba_problem(sc["problem"], "bench_lba")
    T = np.zeros((pr.n_kf, 16), np.float32); X = np.zeros((pr.n_points, 3), np.float32); fl = np.zeros(pr.n_edges, np.uint8)
    rep = pkg.orbx.LbaReport()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    L = pkg.lib()
    call = lambda: L.orbx_local_bundle_adjustment(0, C.byref(pr), None, p(T), p(X), p(fl), None, None, C.byref(rep))
    for _ in range(3):
        if call() != 0:
            raise SystemExit(L.orbx_last_error().decode())
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ts.append(time.perf_counter() - t0)
    dev = 1e3 * float(np.median(ts))
    ntr = sum(rep.trials)
    print(f"free {free} fixed {fixed} points {pr.n_points} edges {pr.n_edges} rows {list(rep.n_active_kf)}: device {dev:9.3f} ms per call "
          f"(iterations {list(rep.iterations)}, trials {list(rep.trials)}, {dev / max(ntr, 1):7.3f} ms per trial, chi2 {rep.chi2[0]:.6g} {rep.chi2[1]:.6g}, "
          f"erased {rep.n_erase})", flush=True)
    names = ["k_lba_init", "k_lba_active", "k_lba_points<true>", "k_lba_kf", "k_lba_reduce", "k_lba_prep", "k_lba_schur", "k_lba_solve", "k_lba_update",
             "k_lba_points<false>", "k_lba_classify", "k_lba_finish"]
    ms = np.zeros(12); cnt = np.zeros(12, np.int32)
    L.orbx_debug_lba_profile(1, None, None)
    for _ in range(5):
        call()
    L.orbx_debug_lba_profile(0, p(ms), p(cnt))
    for k in range(12):
        if cnt[k]:
            print(f"  kernel {names[k]:20s} launches per call {cnt[k] / 5:6.1f}   {1e3 * ms[k] / cnt[k]:9.2f} us per launch   {1e3 * ms[k] / 5 / max(ntr, 1):9.2f} us per trial",
                  flush=True)
    if so:
        H = C.CDLL(so)
        T2 = np.zeros_like(T); X2 = np.zeros_like(X); fl2 = np.zeros_like(fl); tr = (C.c_int * 2)(); chi = (C.c_double * 2)()
        Tin, cam, fx, Xin, ek, ep, mx, my, mr, w = keep
        host = lambda: H.lba_host_loop(pr.n_kf, p(Tin), p(cam), p(fx), pr.n_points, p(Xin), pr.n_edges, p(ek), p(ep), p(mx), p(my), p(mr), p(w),
                                       p(T2), p(X2), p(fl2), tr, chi)
        host()
        ts = []
        for _ in range(max(3, reps // 10)):
            t0 = time.perf_counter()
            host()
            ts.append(time.perf_counter() - t0)
        hst = 1e3 * float(np.median(ts))
        print(f"  host loop, one core: {hst:9.3f} ms per call (trials {list(tr)}, {hst / max(sum(tr), 1):7.3f} ms per trial, chi2 {chi[0]:.6g} {chi[1]:.6g}, "
              f"flags that differ from the device's {int((fl2 != fl).sum())} of {len(fl)})", flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default="")
    ap.add_argument("--step", type=int, default=-1)
    ap.add_argument("so", nargs="?", default="")
    a = ap.parse_args()
    if a.step >= 0:
        return step(a.step, a.reps, a.so)
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

    say(f"# Optimizer::LocalBundleAdjustment on the device, host-inclusive (a clock round the ABI call), medians of {a.reps} calls; device: "
        f"{pkg.orbx.device_identity(0)}")
    say("# the host loop is tools/lba_host_loop.cc on one core: a lower bound for a dense-Schur host solver, NOT the reference (g2o is not built here)")
    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "liblba_host_loop.so")
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++11", "-shared", "-fPIC", os.path.join(ROOT, "tools", "lba_host_loop.cc"), "-o", so])
        for index in range(len(SHAPES)):
            cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--step", str(index), so]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMIT)
            except subprocess.TimeoutExpired:
                say(f"# shape {SHAPES[index]}: no result within {STEP_LIMIT} s; stopping")
                return 1
            if r.returncode != 0:
                say(f"# shape {SHAPES[index]}: exit status {r.returncode}; stopping\n{r.stdout}{r.stderr[-600:]}")
                return 1
            say(r.stdout.rstrip())
    return 0


if __name__ == "__main__":
    sys.exit(main())
