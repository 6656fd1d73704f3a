"""Timing of the panel LDL^T (orbx_ldlt.hip) and of Optimizer::BundleAdjustment on the device (orbx_bundle_adjustment), host-inclusive: a
clock round the ABI call, medians of --reps calls; per-kernel device times through orbx_debug_lba_profile (every launch between two events
and waited for; those calls' wall times are not reported).
  solver     orbx_local_bundle_adjustment on tools/bench_lba.py's windows (10, 30, 100 free keyframes: n = 60, 180, 600) with the
             one-workgroup k_lba_solve (form 0, the kernel as it was before the panels existed) and with the panels (form 1), in the same
             process; the outputs of the two are compared byte for byte.  Then the solve alone through orbx_debug_ldlt_solve on seeded SPD
             systems of growing n, both forms where form 0 exists: the crossover.
  whole call maps of about 50, 300 and 1 000 free keyframes (tests/lba_scene.py's generator, one fixed keyframe, stereo), 10 iterations at
             the most (the _nBad rule ends these maps after 7; the report prints the count).
One condition is enforced: at n = 600 (the window of 100 free keyframes) the panels must solve faster than the one-workgroup kernel, which
uses one compute unit of 256; if they do not, the report says so and the exit status is 1.  Nothing else is gated on these times; g2o
cannot be built here and no speed-up over it is claimed.
  --out F   the report is also written to F (profiles/r21_gba.txt)"""
import argparse
import ctypes as C
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
WINDOWS = [(10, 10, 1000, 8), (30, 30, 3000, 11), (100, 100, 8000, 13)]     # tools/bench_lba.py's: free, fixed, points, the most views of a point
SOLVE_N = [32, 60, 96, 128, 180, 256, 384, 600, 1024, 1536, 3072, 6144]
MAPS = [(50, 4000, 8), (300, 15000, 8), (1000, 40000, 8)]                   # free, points, the most views of a point
NAMES = ["k_lba_init", "active set", "k_lba_points<true>", "k_lba_kf", "k_lba_reduce", "k_lba_prep", "k_lba_schur", "solve", "k_lba_update",
         "k_lba_points<false>", "k_lba_classify", "k_lba_finish"]
STEP_LIMIT = 500
p = lambda a: a.ctypes.data_as(C.c_void_p)


def median_ms(call, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def profile(L, call, calls, trials):
    ms = np.zeros(12); cnt = np.zeros(12, np.int32)
    L.orbx_debug_lba_profile(1, None, None)
    for _ in range(calls):
        call()
    L.orbx_debug_lba_profile(0, p(ms), p(cnt))
    for k in range(12):
        if cnt[k]:
            print(f"  kernel {NAMES[k]:20s} launches per call {cnt[k] / calls:6.1f}   {1e3 * ms[k] / cnt[k]:10.2f} us per launch   "
                  f"{1e3 * ms[k] / calls / max(trials, 1):10.2f} us per trial", flush=True)
    return 1e3 * ms[7] / calls / max(trials, 1)


def step_window(index, reps):
    import __graft_entry__ as ge
    import lba_scene as ls
    pkg = ge.load_pkg()
    L = pkg.lib()
    free, fixed, points, views = WINDOWS[index]
    sc = ls.scene(31 + index, free, fixed, points, "mixed", max_views=views)
    pr, keep = pkg.orbx._lba_problem(sc["problem"], "bench_gba")
    rep = pkg.orbx.LbaReport()
    outs = {}
    for form in (0, 1):
        T = np.zeros((pr.n_kf, 16), np.float32); X = np.zeros((pr.n_points, 3), np.float32); fl = np.zeros(pr.n_edges, np.uint8)
        call = lambda: L.orbx_local_bundle_adjustment(0, C.byref(pr), None, p(T), p(X), p(fl), None, None, C.byref(rep))
        L.orbx_debug_set_lba_solver(form)
        for _ in range(3):
            if call() != 0:
                raise SystemExit(L.orbx_last_error().decode())
        dev = median_ms(call, reps)
        ntr = sum(rep.trials)
        print(f"window free {free} fixed {fixed} points {pr.n_points} edges {pr.n_edges} n {6 * rep.n_active_kf[0]} solver form {form}: {dev:9.3f} ms per call "
              f"(trials {list(rep.trials)}, {dev / max(ntr, 1):7.3f} ms per trial)", flush=True)
        solve = profile(L, call, 5, ntr)
        print(f"  solve, form {form}: {solve:10.2f} us per trial", flush=True)
        outs[form] = (T.tobytes(), X.tobytes(), fl.tobytes())
    L.orbx_debug_set_lba_solver(0)
    print(f"  outputs of the two forms byte-equal: {outs[0] == outs[1]}", flush=True)
    return 0


def step_solve(reps):
    import __graft_entry__ as ge
    pkg = ge.load_pkg()
    L = pkg.lib()
    print(f"solve alone (orbx_debug_ldlt_solve: upload of S, solve, download of x; panel width {L.orbx_debug_ldlt_panel_width()}), medians of {reps} calls; "
          f"'upload' is the same call at a pivot <= 0 in column 0, which solves nothing", flush=True)
    for n in SOLVE_N:
        rng = np.random.Generator(np.random.PCG64(n))
        M = rng.normal(size=(n, n))
        S = M @ M.T + n * np.eye(n); b = rng.normal(size=n); x = np.zeros(n); ok = C.c_int()
        Sbad = S.copy(); Sbad[0, 0] = -1.0
        res = {}
        for form in ((0, 1) if n <= 1536 else (1,)):
            r = max(3, reps if n <= 1536 else reps // 5)
            call = lambda: L.orbx_debug_ldlt_solve(0, n, p(S), p(b), p(x), form, C.byref(ok))
            idle = lambda: L.orbx_debug_ldlt_solve(0, n, p(Sbad), p(b), p(x), form, C.byref(ok))
            call(); idle()
            res[form] = (median_ms(call, r), median_ms(idle, r), x.tobytes())
        line = f"  n {n:5d}:"
        for form, (t, t0, _) in res.items():
            line += f"   form {form} {t:9.3f} ms (upload {t0:8.3f} ms, solve about {t - t0:9.3f} ms)"
        if len(res) == 2:
            line += f"   byte-equal {res[0][2] == res[1][2]}"
        print(line, flush=True)
    return 0


def step_map(index, reps):
    import __graft_entry__ as ge
    import lba_scene as ls
    pkg = ge.load_pkg()
    L = pkg.lib()
    free, points, views = MAPS[index]
    sc = ls.scene(77 + index, free, 1, points, "stereo", max_views=views)
    pr, keep = pkg.orbx._lba_problem(sc["problem"], "bench_gba")
    T = np.zeros((pr.n_kf, 16), np.float32); X = np.zeros((pr.n_points, 3), np.float32); inc = np.zeros(pr.n_points, np.uint8)
    rep = pkg.orbx.BaReport()
    opt = pkg.orbx.BaOptions(None, -1, 10, 1)
    call = lambda: L.orbx_bundle_adjustment(0, C.byref(pr), C.byref(opt), p(T), p(X), p(inc), None, None, C.byref(rep))
    for _ in range(2):
        if call() != 0:
            raise SystemExit(L.orbx_last_error().decode())
    dev = median_ms(call, reps)
    print(f"map free {free} points {pr.n_points} edges {pr.n_edges} rows {rep.n_active_kf} (n = {6 * rep.n_active_kf}): {dev:10.3f} ms per call "
          f"(iterations {rep.iterations}, trials {rep.trials}, {dev / max(rep.trials, 1):9.3f} ms per trial, chi2 {rep.chi2:.6g})", flush=True)
    profile(L, call, 2, rep.trials)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default="")
    ap.add_argument("--step", default="")
    a = ap.parse_args()
    if a.step:
        kind, _, index = a.step.partition(":")
        if kind == "window":
            return step_window(int(index), a.reps)
        if kind == "solve":
            return step_solve(a.reps)
        return step_map(int(index), max(3, a.reps // 6))
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

    say(f"# the panel LDL^T and Optimizer::BundleAdjustment on the device, host-inclusive (a clock round the ABI call), medians of {a.reps} calls "
        f"(whole maps: {max(3, a.reps // 6)}); device: {pkg.orbx.device_identity(0)}")
    say("# solver form 0 = k_lba_solve, one workgroup (unchanged by the panels); form 1 = orbx_ldlt.hip.  g2o is not built here: no speed-up over it is claimed")
    steps = [f"window:{i}" for i in range(len(WINDOWS))] + ["solve:0"] + [f"map:{i}" for i in range(len(MAPS))]
    met = True
    for st in steps:
        cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--step", st]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMIT)
        except subprocess.TimeoutExpired:
            say(f"# step {st}: no result within {STEP_LIMIT} s; stopping")
            return 1
        if r.returncode != 0:
            say(f"# step {st}: exit status {r.returncode}; stopping\n{r.stdout}{r.stderr[-600:]}")
            return 1
        say(r.stdout.rstrip())
        if st == f"window:{len(WINDOWS) - 1}":
            us = {int(f): float(v) for f, v in re.findall(r"solve, form (\d): +([0-9.]+) us per trial", r.stdout)}
            met = us[1] < us[0]
            say(f"# condition: at n = 600 the panels solve in {us[1]:.2f} us per trial, the one-workgroup kernel in {us[0]:.2f} us: {'met' if met else 'NOT MET'}")
    return 0 if met else 1


if __name__ == "__main__":
    sys.exit(main())
