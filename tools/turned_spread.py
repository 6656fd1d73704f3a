"""The largest disagreement of tests/pose_model.py, tests/lba_model.py and tests/gba_model.py with themselves across their three summation
orders, over the scenes in turned world frames and the un-turned halves of the metamorphic pairs (tests/turned_frames.py), in the metrics of tools/pose_spread.py and tools/lba_spread.py.
tests/test_turned_frames.py gives the GPU 64 x this spread.  Also checks the scenes' conditions: every scene admissible (for a half turn
the un-turned scene of the same seed too), every solver in each of the branches 1, 2, 3 of Quaternion(Matrix3), a d22 problem of each bundle
adjustment with keyframes in three branches, and per solver a half-turn scene whose run flips the sign of a quaternion inside pose_mul.
    python tools/turned_spread.py              the spread over the scenes as they are
    python tools/turned_spread.py --select     the *_SEED_SHIFT tables of tests/turned_frames.py (32 shifts at the most)
    python tools/turned_spread.py --mutations  per solver the smallest output change of quat_branch1 / 2 / 3 (pose_model.QUAT_MUTATIONS) over
                                               the turned scenes with a start pose in that branch; what quat_tie_ge and quat_no_flip change"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import gba_model as gm   # noqa: E402
import gba_scene as gs   # noqa: E402
import lba_model as lm   # noqa: E402
import lba_scene as ls   # noqa: E402
import pose_model as pm   # noqa: E402
import pose_scene as ps   # noqa: E402
import turned_frames as tf   # noqa: E402
from tools.gba_spread import CONDITION as GBA_CONDITION   # noqa: E402
from tools.lba_spread import CONDITION as LBA_CONDITION, out_diff, points_diff, poses_diff, up   # noqa: E402
from tools.pose_spread import ORDERS, chi2_diff, pose_diff   # noqa: E402


def pose_run3(sc):
    return [pm.optimize(sc["obs"], sc["cam"], sc["Tcw"], o) for o in ORDERS]


def lba_run3(sc):
    return [lm.optimize(sc["problem"], o) for o in lm.ORDERS]


def gba_run3(sc, opts):
    return [gm.optimize(sc["problem"], order=o, **opts) for o in gm.ORDERS]


def pose_out_diff(a, b):
    return max(pose_diff(a["pose"], b["pose"]), chi2_diff(a["chi2"], b["chi2"]))


def finite(d):
    """a change that is not a number (the mutated run left the reals) counts as an unbounded one"""
    return float(d) if math.isfinite(d) else math.inf


def pose_good(n, sc):
    return ps.admissible(n, sc, pose_run3(sc))


def lba_good(sc):
    rs = lba_run3(sc)
    return ls.admissible(sc, rs) and max(out_diff(rs[0], r) for r in rs[1:]) <= LBA_CONDITION


def gba_good(sc, opts):
    rs = gba_run3(sc, opts)
    return gs.admissible(rs) and max(out_diff(rs[0], r) for r in rs[1:]) <= GBA_CONDITION


def first_shift(good, limit, what):
    for shift in range(limit):
        if good(shift):
            return shift
    raise SystemExit(f"no admissible {what} among {limit} shifts: take the next turn of the same branch")


def select():
    """*_SEED_SHIFT: per case the first of 32 shifts whose turned scene is admissible (for the bundle adjustments tools/lba_spread.py's and
    tools/gba_spread.py's rule, with their bound on the condition).  *_PAIR_SHIFT: per half-turn case whose un-turned scene of that seed is
    not admissible, the first shift at which both are (the metamorphic test runs both sides); monocular pose scenes are the rare ones, as
    the shifts of pose_scene.SEED_SHIFT show, and this search goes as far as tools/pose_spread.py's"""
    seed = dict(pose={}, lba={}, gba={})
    pair = dict(pose={}, lba={}, gba={})
    plain = {}

    def memo(key, fn):
        if key not in plain:
            plain[key] = fn()
        return plain[key]

    def choose(solver, key, turned, untouched):
        shift = first_shift(turned, 32, f"{solver} scene {key}")
        if shift:
            seed[solver][key] = shift
        if key[-1] in tf.HALF_TURNS and not untouched(shift):
            pair[solver][key] = first_shift(lambda s: untouched(s) and turned(s), 1000, f"{solver} pair {key}")

    for n, mix, turn in tf.POSE_CASES:
        choose("pose", (n, mix, turn), lambda s: pose_good(n, tf.pose_case(n, mix, turn, s)),
               lambda s: memo(("pose", n, mix, s), lambda: pose_good(n, tf.pose_case(n, mix, None, s))))
    for shape, mix, turn in tf.LBA_CASES:
        choose("lba", (shape, mix, turn), lambda s: lba_good(tf.lba_case(shape, mix, turn, s)),
               lambda s: memo(("lba", shape, mix, s), lambda: lba_good(tf.lba_case(shape, mix, None, s))))
    for shape, turn in tf.GBA_CASES:
        choose("gba", (shape, turn), lambda s: gba_good(*tf.gba_case(shape, turn, s)),
               lambda s: memo(("gba", shape, s), lambda: gba_good(*tf.gba_case(shape, None, s))))
    for solver in ("pose", "lba", "gba"):
        print(f"{solver.upper()}_SEED_SHIFT =", seed[solver])
    for solver in ("pose", "lba", "gba"):
        print(f"{solver.upper()}_PAIR_SHIFT =", pair[solver])
    return 0


def cases():
    """-> (solver, tag, turn, scene, the branches of its start poses, run(order), whether it is a case of the tables).  The others are the
    scenes of the metamorphic pairs that are no case themselves: the un-turned scene of a half-turn case's seed, and both scenes of a pair
    that needed a shift of its own.  They count for the spread and the condition, not for what the tables have to reach."""
    def pose_entry(tag, turn, sc, case):
        return "pose", tag, turn, sc, [tf.branch_of(sc["Tcw"][:3, :3])], (lambda o: pm.optimize(sc["obs"], sc["cam"], sc["Tcw"], o)), case

    def ba_entry(solver, tag, turn, sc, opts, case):
        run = (lambda o: lm.optimize(sc["problem"], o)) if solver == "lba" else (lambda o: gm.optimize(sc["problem"], order=o, **opts))
        return solver, tag, turn, sc, tf.branches_of_problem(sc["problem"]), run, case

    for n, mix, turn in tf.POSE_CASES:
        tag = tf.pose_tag(n, mix, turn)
        yield pose_entry(tag, turn, tf.pose_case(n, mix, turn), True)
        if turn in tf.HALF_TURNS:
            t, u = tf.pose_pair(n, mix, turn)
            if (n, mix, turn) in tf.POSE_PAIR_SHIFT:
                yield pose_entry(tag + " pair", turn, t, False)
            yield pose_entry(tag + " plain", turn, u, False)
    for shape, mix, turn in tf.LBA_CASES:
        tag = tf.lba_tag(shape, mix, turn)
        yield ba_entry("lba", tag, turn, tf.lba_case(shape, mix, turn), None, True)
        if turn in tf.HALF_TURNS:
            t, u = tf.lba_pair(shape, mix, turn)
            if (shape, mix, turn) in tf.LBA_PAIR_SHIFT:
                yield ba_entry("lba", tag + " pair", turn, t, None, False)
            yield ba_entry("lba", tag + " plain", turn, u, None, False)
    for shape, turn in tf.GBA_CASES:
        tag = tf.gba_tag(shape, turn)
        sc, opts = tf.gba_case(shape, turn)
        yield ba_entry("gba", tag, turn, sc, opts, True)
        if turn in tf.HALF_TURNS:
            t, u = tf.gba_pair(shape, turn)
            if (shape, turn) in tf.GBA_PAIR_SHIFT:
                yield ba_entry("gba", tag + " pair", turn, t, opts, False)
            yield ba_entry("gba", tag + " plain", turn, u, opts, False)


def admissible(solver, tag, sc, rs):
    if solver == "pose":
        return ps.admissible(int(tag.split("-")[0]), sc, rs)
    if solver == "lba":
        return ls.admissible(sc, rs) and max(out_diff(rs[0], r) for r in rs[1:]) <= LBA_CONDITION
    return gs.admissible(rs) and max(out_diff(rs[0], r) for r in rs[1:]) <= GBA_CONDITION


def spread():
    worst = dict(pose=[0.0, 0.0, 0.0], lba=[0.0, 0.0, 0.0], gba=[0.0, 0.0, 0.0])
    reached = dict(pose=set(), lba=set(), gba=set())
    three, mul_flip = set(), set()
    bad = []
    for solver, tag, turn, sc, br, run, case in cases():
        rs = [run(o) for o in ORDERS]
        a = rs[0]
        if solver == "pose":
            dp = max(pose_diff(a["pose"], r["pose"]) for r in rs[1:])
            dx = 0.0
        else:
            dp = max(poses_diff(a["pose"], r["pose"]) for r in rs[1:])
            dx = max(points_diff(a["point"], r["point"]) for r in rs[1:])
        dc = max(chi2_diff(a["chi2"], r["chi2"]) for r in rs[1:])
        ok = admissible(solver, tag, sc, rs)
        flips = a["quat_flips"]
        print(f"{solver:4s} {tag:30s} branches {sorted(set(br))} flips {flips['input']} {flips['exp']} {flips['mul']} admissible {int(ok)} "
              f"pose {dp:.2e} point {dx:.2e} chi2 {dc:.2e}", flush=True)
        if not ok:
            bad.append((solver, tag))
        w = worst[solver]
        w[0], w[1], w[2] = max(w[0], dp), max(w[1], dx), max(w[2], dc)
        if not case:
            continue
        reached[solver] |= set(br)
        if turn == "d22" and len(set(br)) >= 3:
            three.add(solver)
        if turn in tf.HALF_TURNS and flips["mul"] > 0:
            mul_flip.add(solver)
    for solver, w in worst.items():
        w = [up(v) for v in w]
        name = solver.upper()
        if solver == "pose":
            print(f"{name}_SPREAD_POSE = {w[0]:.3e}  {name}_SPREAD_CHI2 = {w[2]:.3e}  (x 64: {64 * w[0]:.3e}, {64 * w[2]:.3e})")
        else:
            print(f"{name}_SPREAD_POSE = {w[0]:.3e}  {name}_SPREAD_POINT = {w[1]:.3e}  {name}_SPREAD_CHI2 = {w[2]:.3e}  "
                  f"(x 64: {64 * w[0]:.3e}, {64 * w[1]:.3e}, {64 * w[2]:.3e})")
    missing = [(s, b) for s in reached for b in (1, 2, 3) if b not in reached[s]]
    print(f"scenes to replace: {bad}  branches not reached: {missing}  d22 problems in three branches: {sorted(three)}  "
          f"half turns that flip inside pose_mul: {sorted(mul_flip)}")
    return 1 if bad or missing or not {"lba", "gba"} <= three or mul_flip != {"pose", "lba", "gba"} else 0


def mutations():
    small = {(s, b): math.inf for s in ("pose", "lba", "gba") for b in (1, 2, 3)}
    count = dict.fromkeys(small, 0)
    no_flip = dict(pose=0.0, lba=0.0, gba=0.0)
    for solver, tag, turn, sc, br, run_order, case in cases():
        if not case:
            continue
        run = lambda: run_order("asc")
        diff = pose_out_diff if solver == "pose" else out_diff
        base = run()
        for b in sorted(set(br) - {0}):
            with pm.quat_mutation(f"quat_branch{b}"), np.errstate(all="ignore"):
                d = finite(diff(base, run()))
            print(f"quat_branch{b} {solver:4s} {tag:24s} change {d:.3e}", flush=True)
            small[(solver, b)] = min(small[(solver, b)], d)
            count[(solver, b)] += 1
        if turn in tf.HALF_TURNS:
            with pm.quat_mutation("quat_no_flip"):
                d = finite(diff(base, run()))
            print(f"quat_no_flip  {solver:4s} {tag:24s} change {d:.3e} flips {base['quat_flips']}", flush=True)
            no_flip[solver] = max(no_flip[solver], d)
    for (solver, b), v in small.items():
        print(f"MUTATION quat_branch{b} {solver} smallest change {v:.3e} over {count[(solver, b)]} scenes")
    ties = 0
    for name, M, _, _ in tf.EXACT_ROTATIONS:
        if name in tf.TIES:
            m = M.astype(np.float64)
            a = pm.quat_to_matrix(pm.quat_normalize(pm.quat_from_matrix(m)))
            with pm.quat_mutation("quat_tie_ge"):
                b_ = pm.quat_to_matrix(pm.quat_normalize(pm.quat_from_matrix(m)))
            ties += a.tobytes() != b_.tobytes()
    print(f"MUTATION quat_tie_ge changes the round trip of {ties} of {len(tf.TIES)} tie matrices")
    print(f"MUTATION quat_no_flip largest change pose {no_flip['pose']:.3e} lba {no_flip['lba']:.3e} gba {no_flip['gba']:.3e} (the same rotation: "
          f"within the spread)")
    for solver in ("pose", "lba", "gba"):
        print(f"{solver.upper()}_SMALLEST_MUTATION = {min(small[(solver, b)] for b in (1, 2, 3)):.3e}")
    return 0 if all(count[k] > 0 and v > 0.0 for k, v in small.items()) and ties > 0 else 1


def main():
    if "--select" in sys.argv:
        return select()
    if "--mutations" in sys.argv:
        return mutations()
    return spread()


if __name__ == "__main__":
    sys.exit(main())
