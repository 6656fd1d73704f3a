#!/usr/bin/env python3
"""Float Horn + Jacobi against float64: the largest relative difference between the model's s, R, t (tests/sim3_model.py: the contract of
include/orbx.h, float Jacobi on N) and the exact Horn formulas in float64 with numpy.linalg.eigh on the SAME float inputs, over every
sample row of the test suite (tests/sim3_scene.py) whose three points are not near-collinear.  Relative means |ds| / |s|, |dR|_F / |R|_F
and |dt| / |O1| (t is a difference of quantities of the centroid's size).  A triple counts as near-collinear when the sine of the
smallest angle of its triangle, in either camera, is below CUT_OFF: the two largest eigenvalues of N then approach each other and the
rotation about the line is undetermined.  tests/test_sim3_model.py holds the printed value as a constant, with a margin of 16.
Needs no GPU.

    python tools/sim3_spread.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sim3_model as sm      # noqa: E402
import sim3_scene as sc      # noqa: E402

CUT_OFF = 0.05


def spread():
    """-> (largest relative difference, hypotheses compared, hypotheses left out as near-collinear)"""
    worst, count, left_out = 0.0, 0, 0
    for key in sc.keys():
        j = sc.job(*key)
        for row in j["samples"]:
            P1, P2 = j["X1"][row], j["X2"][row]
            if min(sm.collinearity(P1), sm.collinearity(P2)) < CUT_OFF:
                left_out += 1
                continue
            h = sm.horn(P1, P2, j["fix_scale"])
            s, R, t, _w = sm.horn_f64(P1, P2, j["fix_scale"])
            o1 = np.linalg.norm(np.asarray(P1, np.float64).mean(0))
            rel = max(abs(float(h["s"]) - s) / abs(s), float(np.linalg.norm(np.array(h["R"], np.float64) - R) / np.linalg.norm(R)),
                      float(np.linalg.norm(np.array(h["t"], np.float64) - t) / o1))
            worst = max(worst, rel)
            count += 1
    return worst, count, left_out


if __name__ == "__main__":
    w, c, o = spread()
    print(f"hypotheses compared: {c}\nleft out as near-collinear (cut-off {CUT_OFF}): {o} ({100.0 * o / (c + o):.2f} %)\n"
          f"largest relative difference to float64: {w:.3e}")
