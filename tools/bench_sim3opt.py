"""Host-inclusive timing of orbx_sim3_optimize and orbx_sim3_optimize_batch through the Python mirror: medians of 200 calls at 30, 100 and 300
correspondences, single and as a batch of 8 candidates.  The clock holds the staging, the upload, the launch, the download and the mirror's
own argument handling.  No profiler is nested inside it.  Reported, not gated; no figure of the reference stands beside it (g2o cannot be
built here).
    python tools/bench_sim3opt.py"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge   # noqa: E402
import sim3opt_scene as ss     # noqa: E402

REPS, BATCH = 200, 8


def median_us(fn):
    fn()
    t = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)) * 1e6


def main():
    pkg = ge.load_pkg()
    print(f"orbx_sim3_optimize, host-inclusive medians of {REPS} calls (us); batch = {BATCH} candidates in one launch")
    for n in (30, 100, 300):
        scs = [ss.scene(7000 + 10 * n + j, n, "outliers") for j in range(BATCH)]
        r = pkg.sim3_optimize(*ss.args(scs[0]))
        single = median_us(lambda: pkg.sim3_optimize(*ss.args(scs[0])))
        jobs = [ss.args(sc) for sc in scs]
        batch = median_us(lambda: pkg.sim3_optimize_batch(jobs))
        print(f"n_corr {n:4d}: single {single:8.1f}   batch {batch:8.1f} ({batch / BATCH:7.1f} per candidate)   "
              f"[rounds {r['rounds']} n_bad {r['n_bad']} iterations {list(map(int, r['iterations']))} inliers {r['n_inliers']}]")


if __name__ == "__main__":
    main()
