"""The largest disagreement of tests/lba_model.py with itself across its three summation orders, over every scene of the local bundle
adjustment tests (tests/lba_scene.py), in tools/pose_spread.py's metric: per pose entry relative to its block's largest magnitude (rotation
block, translation column), per point relative to the point's norm, per chi2 relative to max(chi2, 1).  tests/test_lba.py gives the GPU
64 x this spread.  Also checks the scenes' condition (lba_scene.admissible).
    python tools/lba_spread.py              the spread over the scenes as they are
    python tools/lba_spread.py --select     the SEED_SHIFT / SPECIAL_SHIFT / DROPPED tables of tests/lba_scene.py (32 shifts at the most)
    python tools/lba_spread.py --mutations  the smallest output change, over the scenes a mutation can touch, of each deliberate error
                                            in the model (lba_model.MUTATIONS)"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import lba_model as lm   # noqa: E402
import lba_scene as ls   # noqa: E402
from tools.pose_spread import chi2_diff, pose_diff   # noqa: E402


def poses_diff(a, b):
    return max([pose_diff(a[k], b[k]) for k in range(len(a))] or [0.0])


def points_diff(a, b):
    if len(a) == 0:
        return 0.0
    return float((np.abs(a - b).max(axis=1) / np.maximum(np.linalg.norm(a, axis=1), 1e-300)).max())


def out_diff(a, b):
    """the largest of the three measures between two results"""
    return max(poses_diff(a["pose"], b["pose"]), points_diff(a["point"], b["point"]), chi2_diff(a["chi2"], b["chi2"]))


def run3(sc, **kw):
    return [lm.optimize(sc["problem"], o, **kw) for o in lm.ORDERS]


CONDITION = 1e-11   # --select: a scene whose three orders disagree by more than this is too ill-conditioned to pin anything: the next seed


def good(sc):
    rs = run3(sc)
    return ls.admissible(sc, rs) and max(out_diff(rs[0], r) for r in rs[1:]) <= CONDITION


def select():
    shifts, dropped, special = {}, [], {}
    for shape in ls.SHAPES:
        for mix in ls.MIXES:
            for shift in range(32):
                sc = ls.shape_scene(shape, mix, shift)
                if good(sc):
                    if shift:
                        shifts[(shape, mix)] = shift
                    break
            else:
                dropped.append((shape, mix))
    for name in ls.SPECIAL:
        for shift in range(32):
            sc = ls.special_scene(name, shift)
            if good(sc):
                if shift:
                    special[name] = shift
                break
        else:
            raise SystemExit(f"no admissible special scene {name}")
    print("SEED_SHIFT =", shifts)
    print("SPECIAL_SHIFT =", special)
    print("DROPPED =", set(dropped) or "set()")


def up(v):
    """v rounded up in the fourth digit"""
    if v <= 0:
        return 0.0
    r = float(f"{v:.3e}")
    return r if r >= v else r + 10.0 ** (math.floor(math.log10(v)) - 3)


def mutations():
    worst, touched = {}, {}
    for m in lm.MUTATIONS:
        small = math.inf
        for tag, sc in ls.all_scenes():
            pr = sc["problem"]
            if len(pr["edge_kf"]) == 0:
                continue
            if m == "invz_double" and not (pr["u_right"] >= 0).any():
                continue
            base = lm.optimize(pr, "asc")
            mut = lm.optimize(pr, "asc", mutation=m)
            d = out_diff(base, mut)
            flags = int((base["edge_flags"] != mut["edge_flags"]).sum())
            print(f"{m:15s} {tag:22s} change {d:.3e} flags changed {flags}")
            if m == "reeval_level1":          # it changes flags, never estimates: the exact comparison of the flags is what catches it
                touched[m] = touched.get(m, 0) + (flags > 0)
                continue
            if m == "lambda_poses" and mut["lambda_init"] == base["lambda_init"]:
                continue                      # the largest diagonal entry is a pose's in both rounds: the error cannot show in this scene
            touched[m] = touched.get(m, 0) + 1
            small = min(small, d)
        worst[m] = small
    for m, v in worst.items():
        print(f"MUTATION {m} smallest change {v:.3e} over {touched.get(m, 0)} scenes")
    numeric = {m: v for m, v in worst.items() if m != "reeval_level1"}
    print(f"SMALLEST_MUTATION = {min(numeric.values()):.3e}")
    # every listed error must show somewhere: a numeric one in a finite change, the flag one in changed flags
    return 0 if all(math.isfinite(v) for v in numeric.values()) and touched.get("reeval_level1", 0) > 0 else 1


def main():
    if "--select" in sys.argv:
        return select()
    if "--mutations" in sys.argv:
        return mutations()
    wp = wx = wc = 0.0
    bad = []
    for tag, sc in ls.all_scenes():
        rs = run3(sc)
        a = rs[0]
        dp = max(poses_diff(a["pose"], r["pose"]) for r in rs[1:])
        dx = max(points_diff(a["point"], r["point"]) for r in rs[1:])
        dc = max(chi2_diff(a["chi2"], r["chi2"]) for r in rs[1:])
        ok = ls.admissible(sc, rs)
        print(f"{tag:22s} active kf {a['n_active_kf']} points {a['n_active_points']} iterations {a['iterations']} trials {a['trials']} level1 {a['n_level1']} "
              f"erase {a['n_erase']} chi2 {a['chi2'][0]:.4g} {a['chi2'][1]:.4g} admissible {int(ok)} pose {dp:.2e} point {dx:.2e} chi2 {dc:.2e}")
        if not ok:
            bad.append(tag)
        wp, wx, wc = max(wp, dp), max(wx, dx), max(wc, dc)
    wp, wx, wc = up(wp), up(wx), up(wc)
    print(f"SPREAD_POSE = {wp:.3e}  SPREAD_POINT = {wx:.3e}  SPREAD_CHI2 = {wc:.3e}  (x 64: {64 * wp:.3e}, {64 * wx:.3e}, {64 * wc:.3e})  scenes to replace: {bad}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
