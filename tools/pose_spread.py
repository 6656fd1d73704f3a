"""The largest disagreement of tests/pose_model.py with itself across its three summation orders, over every scene of the PoseOptimization
GPU tests (tests/pose_scene.py): per pose entry relative to its block's largest magnitude (rotation, translation), and per chi2 relative to
max(chi2, 1).  tests/test_pose_opt.py gives the GPU 64 x this spread.  Also checks the scenes' condition (pose_scene.admissible).
    python tools/pose_spread.py            the spread over the scenes as they are
    python tools/pose_spread.py --select   the SEED_SHIFT table of tests/pose_scene.py"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pose_model as pm   # noqa: E402
import pose_scene as ps   # noqa: E402


def pose_diff(a, b):
    """per-entry |a - b| relative to the block's largest magnitude -> the largest"""
    d = np.abs(a - b)
    r = d[:, :3].max() / np.abs(a[:, :3]).max()
    t = d[:, 3].max() / max(np.abs(a[:, 3]).max(), 1e-300)
    return max(r, t)


def chi2_diff(a, b):
    # relative to max(chi2, 1): three monocular points are fitted exactly, their chi2 is rounding residue (1e-20) and has no relative
    # accuracy; what a chi2 is compared with is a threshold of 5.991 / 7.815, so below 1 the scale that matters is 1
    a, b = np.asarray(a), np.asarray(b)
    return float((np.abs(a - b) / np.maximum(np.abs(a), 1.0)).max())


ORDERS = ("asc", "desc", "pair")


def select():
    """-> the SEED_SHIFT table of tests/pose_scene.py: per scene the first shift whose scene is admissible"""
    table = {}
    for n in ps.SIZES:
        for mix in ps.MIXES:
            for shift in range(1000):
                sc = ps.scene(1000 * ps.MIXES.index(mix) + n + 5000 * shift, n, mix)
                if ps.admissible(n, sc, [pm.optimize(sc["obs"], sc["cam"], sc["Tcw"], o) for o in ORDERS]):
                    break
            else:
                raise SystemExit(f"no admissible scene for {n} {mix}")
            if shift:
                table[(n, mix)] = shift
    print("SEED_SHIFT =", table)


def main():
    if "--select" in sys.argv:
        return select()
    worst_p = worst_c = 0.0
    bad = []
    for n, mix, sc in ps.all_scenes():
        rs = [pm.optimize(sc["obs"], sc["cam"], sc["Tcw"], o) for o in ORDERS]
        a = rs[0]
        dp = max(pose_diff(a["pose"], r["pose"]) for r in rs[1:])
        dc = max(chi2_diff(a["chi2"], r["chi2"]) for r in rs[1:])
        ok = ps.admissible(n, sc, rs)
        print(f"n {n:5d} {mix:6s} rounds {a['rounds']} n_bad {a['n_bad']} iterations {a['iterations']} admissible {int(ok)} pose {dp:.2e} chi2 {dc:.2e}"
              f" stale {int(a['stale_used'])}")
        if not ok:
            bad.append((n, mix))
        worst_p, worst_c = max(worst_p, dp), max(worst_c, dc)
    up = lambda v: float(f"{v:.3e}") + (10.0 ** (math.floor(math.log10(v)) - 3) if v > 0 and float(f"{v:.3e}") < v else 0.0)   # never below
    worst_p, worst_c = up(worst_p), up(worst_c)
    print(f"SPREAD_POSE = {worst_p:.3e}  SPREAD_CHI2 = {worst_c:.3e}  (x 64: {64 * worst_p:.3e}, {64 * worst_c:.3e})  scenes to replace: {bad}")
    return 1 if bad or 64 * max(worst_p, worst_c) >= 1e-9 else 0


if __name__ == "__main__":
    sys.exit(main())
