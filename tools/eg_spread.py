"""The largest disagreement of tests/eg_model.py with itself across its variants -- the three summation orders, two seeded one-ulp nudges
of sin / cos / exp / log / acos, and the closed-form Jacobian in place of the central difference -- over every scene of the
OptimizeEssentialGraph tests (tests/eg_scene.py): every keyframe's Sim3 as [s R | t] in tools/sim3opt_spread.py's s12_diff, the corrected
points in tools/lba_spread.py's points_diff, chi2 in tools/pose_spread.py's chi2_diff.  tests/test_essential_graph.py gives the GPU 64 x
this spread.
    python tools/eg_spread.py              SPREAD_S, SPREAD_POINT, SPREAD_CHI2 over the scenes as they are
    python tools/eg_spread.py --mutations  the smallest output change of each deliberate error in the model (eg_model.MUTATIONS), over the
                                           scenes the error can touch
    python tools/eg_spread.py --stages     per case of eg_scene.STAGE_CASES and per row of err (of the trial estimates for an exp table) the
                                           model's spread across nudge None, 1, 2 (tests/eg_stage_checks.py: row_bounds), the floor, the
                                           rows whose bound exceeds 1e-10, the paths the case visits; then per mutation the check that
                                           sees it and, for those seen under the bound, the smallest change over the rows it can touch"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import eg_model as em   # noqa: E402
import eg_scene as es   # noqa: E402
from tools.lba_spread import points_diff, poses_diff, up   # noqa: E402
from tools.pose_spread import chi2_diff   # noqa: E402
from tools.sim3opt_spread import s12_diff   # noqa: E402


def s_diff(A, B):
    """the largest s12_diff over the keyframes"""
    return max(s12_diff(a, b) for a, b in zip(A, B))


def out_diff(a, b):
    return max(s_diff(a["S"], b["S"]), poses_diff(a["pose"], b["pose"]), points_diff(a["point"], b["point"]), chi2_diff(a["chi2"], b["chi2"]))


def touches(m, pr, opts):
    """can mutation m change anything in this scene?"""
    if len(pr["edge_i"]) == 0 or opts["iterations"] == 0:
        return m == "t_not_divided" and (pr["S_corrected"][:, 7] != 1.0).any()
    if m == "x6_not_zeroed":
        return bool(pr["fix_scale"])
    if m == "normal_from_vscw":
        kind, non = pr["edge_kind"], pr["noncorrected"]
        return bool(((kind != 0) & ((non[pr["edge_i"]] >= 0) | (non[pr["edge_j"]] >= 0))).any())
    if m == "bta_untransposed":
        fixed = pr["fixed"] != 0
        return bool(((pr["edge_i"] < pr["edge_j"]) & ~fixed[pr["edge_i"]] & ~fixed[pr["edge_j"]]).any())
    if m == "t_not_divided":
        return not pr["fix_scale"]
    return True


def mutations(tags):
    worst, touched = {}, {}
    for m in em.MUTATIONS:
        small = math.inf
        for tag in tags:
            pr, opts = es.case(tag)
            if not touches(m, pr, opts):
                continue
            base = em.optimize(pr, **opts)
            mut = em.optimize(pr, mutation=m, **opts)
            d = out_diff(base, mut)
            print(f"{m:17s} {tag:22s} change {d:.3e}", flush=True)
            touched[m] = touched.get(m, 0) + 1
            small = min(small, d)
        worst[m] = small
    for m, v in worst.items():
        print(f"MUTATION {m} smallest change {v:.3e} over {touched.get(m, 0)} scenes")
    print(f"SMALLEST_MUTATION = {min(worst.values()):.3e}")
    return 0 if all(math.isfinite(v) for v in worst.values()) else 1


def stages():
    import eg_stage_checks as ck
    ok = True
    for name in es.STAGE_CASES:
        c, runs = es.stage_case(name), es.stage_models(name)
        q = "trial" if name.startswith("exp-") else "err"
        bound, spread, floor = ck.row_bounds([r[q] for r in runs])
        big = np.nonzero(bound > 1e-10)[0]
        m = runs[0]
        print(f"STAGE {name:28s} {q:5s} rows {len(bound):3d} floor {floor:.3e} largest spread {spread.max():.3e} largest bound {bound.max():.3e} "
              f"rows over 1e-10: {len(big)} ({100.0 * len(big) / len(bound):.1f} %)  log {m['branches']} pivot {m['paths']['pivot']} "
              f"second {m['paths']['second']} exp {m['paths']['exp']} quat {m['paths']['quat']}")
        for i in big:
            print(f"    ROW {i} ({c['labels'][i]}) spread {spread[i]:.3e} bound {bound[i]:.3e}")
        ok = ok and len(big) <= 0.02 * len(bound)
    for mut, (check, kind) in ck.SEEN_BY.items():
        for name in ck.MUTATION_CASES[mut]:
            c, runs = es.stage_case(name), es.stage_models(name)
            bad = es.stage_models(name, mut)[0]
            if kind == "bytes":
                found = ck.run_check(check, c["problem"], bad, c["lam"], runs[0])
                print(f"MUTATION {mut:22s} {name:24s} check {check:8s} bytes: {found[0] if found else 'NOT SEEN'}")
                ok = ok and bool(found)
            else:
                rows, ratio, change, bound = ck.margin(mut, runs, bad)
                print(f"MUTATION {mut:22s} {name:24s} check {check:8s} bound: {len(rows)} rows, smallest change {change:.3e}, largest bound there "
                      f"{bound:.3e}, smallest change / bound {ratio:.3e}")
                ok = ok and len(rows) > 0 and ratio >= 16
    return 0 if ok else 1


def main():
    if "--mutations" in sys.argv:
        return mutations(es.all_tags())
    if "--stages" in sys.argv:
        return stages()
    ws = wx = wc = 0.0
    total = [0, 0, 0, 0]
    for tag in es.all_tags():
        pr, opts = es.case(tag)
        rs = es.variants(pr, opts)
        a = rs[0]
        ds = max(s_diff(a["S"], r["S"]) for r in rs[1:])
        dx = max(points_diff(a["point"], r["point"]) for r in rs[1:])
        dc = max(chi2_diff(a["chi2"], r["chi2"]) for r in rs[1:])
        total = [p + q for p, q in zip(total, a["branches"])]
        print(f"{tag:22s} free {a['n_free']:3d} edges {len(pr['edge_i']):3d} iterations {[r['iterations'] for r in rs]} trials {[r['trials'] for r in rs]} "
              f"chi2 {a['chi2_start']:.4g} -> {a['chi2']:.4g} log branches {a['branches']} S {ds:.2e} point {dx:.2e} chi2 {dc:.2e}", flush=True)
        ws, wx, wc = max(ws, ds), max(wx, dx), max(wc, dc)
    ws, wx, wc = up(ws), up(wx), up(wc)
    print(f"LOG_BRANCHES = {total}")
    print(f"SPREAD_S = {ws:.3e}  SPREAD_POINT = {wx:.3e}  SPREAD_CHI2 = {wc:.3e}  (x 64: {64 * ws:.3e}, {64 * wx:.3e}, {64 * wc:.3e})")
    return 0 if all(total) else 1


if __name__ == "__main__":
    sys.exit(main())
