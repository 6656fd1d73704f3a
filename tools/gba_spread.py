"""The largest disagreement of tests/gba_model.py with itself across its three summation orders, over every scene of the global bundle
adjustment tests (tests/gba_scene.py), in tools/lba_spread.py's metric: per pose entry relative to its block's largest magnitude, per
point relative to the point's norm, per chi2 relative to max(chi2, 1).  tests/test_gba.py gives the GPU 64 x this spread.  Also checks
the scenes' condition (gba_scene.admissible).
    python tools/gba_spread.py              the spread over the scenes as they are (the 260-keyframe scene takes about 17 s per order)
    python tools/gba_spread.py --select     the SEED_SHIFT table of tests/gba_scene.py (32 shifts at the most)
    python tools/gba_spread.py --mutations  the smallest output change, over the scenes a mutation can touch, of each deliberate error
                                            in the model (gba_model.MUTATIONS); the 260-keyframe scene is left out of this one
    --small                                 without the 260-keyframe scene"""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import gba_model as gm   # noqa: E402
import gba_scene as gs   # noqa: E402
from tools.lba_spread import out_diff, points_diff, poses_diff, up   # noqa: E402
from tools.pose_spread import chi2_diff   # noqa: E402

CONDITION = 1e-10   # --select: a scene whose three orders disagree by more than this is too ill-conditioned to pin anything: the next seed


def run3(sc, opts, **kw):
    return [gm.optimize(sc["problem"], order=o, **opts, **kw) for o in gm.ORDERS]


def select(tags):
    shifts = {}
    for tag in tags:
        for shift in range(32):
            sc, opts = gs.case(tag, shift)
            rs = run3(sc, opts)
            if gs.admissible(rs) and max(out_diff(rs[0], r) for r in rs[1:]) <= CONDITION:
                if shift:
                    shifts[tag] = shift
                break
        else:
            raise SystemExit(f"no admissible scene {tag}")
    print("SEED_SHIFT =", shifts)
    return 0


def mutations(tags):
    worst, touched = {}, {}
    for m in gm.MUTATIONS:
        small = math.inf
        for tag in tags:
            sc, opts = gs.case(tag)
            pr = sc["problem"]
            if len(pr["edge_kf"]) == 0 or opts["iterations"] == 0:
                continue
            if m == "invz_double" and not (pr["u_right"] >= 0).any():
                continue
            if m in ("no_huber", "huber_5991") and not opts["robust"]:
                continue
            if m == "huber_5991" and not (pr["u_right"] < 0).any():
                continue
            base = gm.optimize(pr, order="asc", **opts)
            mut = gm.optimize(pr, order="asc", mutation=m, **opts)
            d = out_diff(base, mut)
            print(f"{m:15s} {tag:22s} change {d:.3e}")
            if m == "lambda_poses" and mut["lambda_init"] == base["lambda_init"]:
                continue                      # the largest diagonal entry is a pose's: the error cannot show in this scene
            touched[m] = touched.get(m, 0) + 1
            small = min(small, d)
        worst[m] = small
    for m, v in worst.items():
        print(f"MUTATION {m} smallest change {v:.3e} over {touched.get(m, 0)} scenes")
    print(f"SMALLEST_MUTATION = {min(worst.values()):.3e}")
    return 0 if all(math.isfinite(v) for v in worst.values()) else 1   # every listed error must show somewhere


def main():
    small = "--small" in sys.argv
    if "--select" in sys.argv:
        return select(gs.all_tags(big=not small))
    if "--mutations" in sys.argv:
        return mutations(gs.all_tags(big=False))
    wp = wx = wc = 0.0
    bad = []
    for tag in gs.all_tags(big=not small):
        sc, opts = gs.case(tag)
        rs = run3(sc, opts)
        a = rs[0]
        dp = max(poses_diff(a["pose"], r["pose"]) for r in rs[1:])
        dx = max(points_diff(a["point"], r["point"]) for r in rs[1:])
        dc = max(chi2_diff(a["chi2"], r["chi2"]) for r in rs[1:])
        ok = gs.admissible(rs)
        print(f"{tag:22s} active kf {a['n_active_kf']} points {a['n_active_points']} edges {len(sc['problem']['edge_kf'])} iterations {a['iterations']} "
              f"trials {a['trials']} chi2 {a['chi2']:.4g} admissible {int(ok)} pose {dp:.2e} point {dx:.2e} chi2 {dc:.2e}", flush=True)
        if not ok:
            bad.append(tag)
        wp, wx, wc = max(wp, dp), max(wx, dx), max(wc, dc)
    wp, wx, wc = up(wp), up(wx), up(wc)
    print(f"SPREAD_POSE = {wp:.3e}  SPREAD_POINT = {wx:.3e}  SPREAD_CHI2 = {wc:.3e}  (x 64: {64 * wp:.3e}, {64 * wx:.3e}, {64 * wc:.3e})  scenes to replace: {bad}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
