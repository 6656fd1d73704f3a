#!/usr/bin/env python3
"""Float Jacobi against a double SVD: the largest relative difference |x3D_model - x3D_svd| / |x3D_svd| over the accepted triangulations
(status 0 or 32) of the test suite, where x3D_svd is the null vector of the SAME float matrix A by a float64 numpy.linalg.svd.
tests/test_triangulate_model.py holds the printed value as a constant, with a margin of 16.  Needs no GPU.

    python tools/tri_spread.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import triangulate_model as tm      # noqa: E402
import triangulate_scene as ts      # noqa: E402


def spread():
    """-> (largest relative difference, accepted triangulations, smallest parallax among them in degrees)"""
    worst, count, min_par = 0.0, 0, 180.0
    for s, (status, x3d, _n) in ts.suite():
        for i in range(len(s["k2s"])):
            for k in range(int(s["npairs"][i])):
                if status[i][k] not in (0, 32):
                    continue
                info = {}
                i1, i2 = int(s["pairs"][i][2 * k]), int(s["pairs"][i][2 * k + 1])
                tm.test_pair(s["v1"], s["k1"], i1, s["v2s"][i], s["k2s"][i], i2, s["sf"], s["sigma2"], s["ratio_factor"], info)
                ref = tm.svd_null_point(info["A"])
                worst = max(worst, float(np.linalg.norm(x3d[i][k].astype(np.float64) - ref) / np.linalg.norm(ref)))
                min_par = min(min_par, float(np.degrees(np.arccos(min(1.0, float(info["cos_rays"]))))))
                count += 1
    return worst, count, min_par


if __name__ == "__main__":
    w, c, p = spread()
    print(f"accepted triangulations: {c}\nsmallest parallax: {p:.3f} deg\nlargest relative difference to the float64 SVD: {w:.3e}")
