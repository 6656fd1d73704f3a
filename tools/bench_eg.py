"""Timing of Optimizer::OptimizeEssentialGraph on the device (orbx_optimize_essential_graph, orbx_optimize_essential_graph2), host-inclusive: a
clock round the ABI call, medians of --reps calls, on loops of 100, 500 and 1500 free keyframes, and of 4000 for the envelope solver
(tests/eg_scene.py's generator, fixed scale, so that the call runs its iterations instead of stalling in Sim3::log's faulty branch; about 3
map points a keyframe); per-kernel device times through orbx_debug_eg_profile in calls of their own (every launch between two events and
waited for; those calls' wall times are not reported).  Reported, not gated.  There is no reference figure: g2o cannot be built here, and
nothing in this repository has timed it.
  --solver S  old (orbx_optimize_essential_graph, the default), dense, envelope or auto (orbx_optimize_essential_graph2)
  --out F     the report is also written to F (profiles/r22_eg.txt, profiles/r23_eg_envelope.txt)"""
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
SIZES = [100, 500, 1500, 4000]       # the last one: beyond the dense solve, for the envelope solver alone
SOLVERS = {"old": None, "dense": 0, "envelope": 1, "auto": 2}
NAMES = ["k_eg_setup", "k_eg_edges<true>", "k_eg_rows", "k_eg_reduce", "fill", "solve", "k_eg_update", "k_eg_edges<false>",
         "k_eg_finish", "k_eg_points"]
STEP_LIMIT = 500
p = lambda a: a.ctypes.data_as(C.c_void_p)


def sizes(solver):
    return SIZES if solver in ("envelope", "auto") else SIZES[:3]


def solve_launches(problem, envelope, W=32):
    """kernel launches of one solve, from the structure alone: per panel the diagonal block, then the rows and the trailing update where
    the panel has a row below it (dense: every panel but the last; envelope: a panel with an active row), the scaling, and a launch per
    panel on the way back"""
    fixed = np.asarray(problem["fixed"]) != 0
    F = int((~fixed).sum())
    n = 7 * F
    panels = (n + W - 1) // W
    if not envelope:
        return panels + 2 * ((n - 1) // W) + 1 + panels
    row = np.full(len(fixed), -1)
    row[~fixed] = np.arange(F)
    lowest = np.arange(F)
    ri, rj = row[problem["edge_i"]], row[problem["edge_j"]]
    both = (ri >= 0) & (rj >= 0)
    np.minimum.at(lowest, np.maximum(ri, rj)[both], np.minimum(ri, rj)[both])
    first = np.repeat(7 * lowest // W * W, 7)
    mark = np.zeros(panels + 1, np.int64)                # row i is active in the panels first[i] / W .. i / W - 1
    np.add.at(mark, first // W, 1)
    np.add.at(mark, np.arange(n) // W, -1)
    return panels + 2 * int((np.cumsum(mark)[:panels] > 0).sum()) + 1 + panels


def step(index, reps, solver="old"):
    import __graft_entry__ as ge
    import eg_scene as es
    pkg = ge.load_pkg()
    L = pkg.lib()
    F = SIZES[index]
    scene = es.make(F, 1, 5100 + F)
    pr, keep = pkg.orbx._eg_problem(scene, "bench_eg")
    T = np.zeros((pr.n_kf, 16), np.float32); X = np.zeros((pr.n_points, 3), np.float32)
    rep = pkg.orbx.EgReport()
    if SOLVERS[solver] is None:
        opt = pkg.orbx.EgOptions(20)
        call = lambda: L.orbx_optimize_essential_graph(0, C.byref(pr), C.byref(opt), p(T), p(X), None, None, C.byref(rep))
    else:
        opt = pkg.orbx.EgOptions2(20, SOLVERS[solver])
        call = lambda: L.orbx_optimize_essential_graph2(0, C.byref(pr), C.byref(opt), p(T), p(X), None, None, C.byref(rep))
    entries, triangle = C.c_int64(), C.c_int64()
    L.orbx_eg_envelope(C.byref(pr), C.byref(entries), C.byref(triangle))
    for _ in range(2):
        if call() != 0:
            raise SystemExit(L.orbx_last_error().decode())
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ts.append(time.perf_counter() - t0)
    dev = 1e3 * float(np.median(ts))
    print(f"loop free {F} (n = {7 * F}, S {8 * (7 * F) ** 2 / 1e6:.0f} MB dense, envelope {8 * entries.value / 1e6:.1f} MB = "
          f"{100 * entries.value / max(triangle.value, 1):.2f} % of the triangle) edges {pr.n_edges} points {pr.n_points}: {dev:10.3f} ms per call (iterations "
          f"{rep.iterations}, trials {rep.trials}, failed solves {rep.n_solve_failed}, {dev / max(rep.trials, 1):9.3f} ms per trial, chi2 "
          f"{rep.chi2_start:.4g} -> {rep.chi2:.4g})", flush=True)
    ms = np.zeros(10); cnt = np.zeros(10, np.int32)
    L.orbx_debug_eg_profile(1, None, None)
    call()
    L.orbx_debug_eg_profile(0, p(ms), p(cnt))
    env = SOLVERS[solver] == 1 or (SOLVERS[solver] == 2 and (F > 1536 or 2 * entries.value <= triangle.value))
    print(f"  solver {'envelope' if env else 'dense'}: {solve_launches(scene, env)} launches per solve, {cnt[5]} solves per call", flush=True)
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
    ap.add_argument("--solver", default="old", choices=sorted(SOLVERS))
    a = ap.parse_args()
    if a.step:
        return step(int(a.step), a.reps, a.solver)
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
    say(f"# solver: {a.solver}" + ("" if SOLVERS[a.solver] is None else " (orbx_optimize_essential_graph2)") +
        "; `solves` counts calls of the solver, each of `launches per solve` kernel launches")
    for i in range(len(sizes(a.solver))):
        cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--step", str(i), "--solver", a.solver]
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
