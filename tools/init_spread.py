#!/usr/bin/env python3
"""The Initializer model's float Jacobi against float64, and its recovered motion against the scenes' own.

null vectors: for every sample row of the test suite (tests/init_scene.py) the model's null vector of the 16 x 9 (H) and the 8 x 9 (F)
system (tests/init_model.py: the one-sided float Jacobi of the contract of include/orbx.h) against numpy.linalg.svd in float64 on the
SAME float matrix: the largest component of v_model -/+ v_f64 (the sign is free).  A row is left out when the two smallest of the nine
singular values (the ninth of the 8 x 9 system is 0) are closer than RATIO, s8 > RATIO * s7: the null vector is then undetermined.  That
is a condition on the float64 values alone.

motion: on the noise-free twins of the two scenes that must initialise (general, planar; the keypoints still rounded to float), the
angle between the model's R21 and the scene's rotation and between t21 and the scene's translation direction, in degrees (the scale of
t is free).  With pixel noise the error is the noise's, not the arithmetic's, and 64 times it would bound nothing.

tests/test_init_model.py holds the printed values as constants, with a margin of 64.  Needs no GPU.

    python tools/init_spread.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import init_model as im      # noqa: E402
import init_scene as sc      # noqa: E402

RATIO = 0.5


def systems(key):
    """the float systems of every sample row of a job: (A_h[n_hyp][16][9], A_f[n_hyp][8][9])"""
    sp, _, _ = im.sample_points(sc.job(*key))
    return im.system_h(sp), im.system_f(sp)


def null_f64(A):
    """-> (the null vector in float64, s8 / s7 with s8 = 0 for fewer than nine rows)"""
    _, s, vt = np.linalg.svd(np.asarray(A, np.float64), full_matrices=True)
    s = np.concatenate([s, np.zeros(9 - len(s))])
    return vt[8], (s[8] / s[7] if s[7] > 0 else 1.0)


def null_spread():
    """-> (largest disagreement, rows compared, rows left out)"""
    worst, count, left_out = 0.0, 0, 0
    for key in sc.keys():
        for A in systems(key):
            got = im.null_of(A)[0].astype(np.float64)
            for h in range(len(A)):
                ref, ratio = null_f64(A[h])
                if ratio > RATIO:
                    left_out += 1
                    continue
                v = got[h] / np.linalg.norm(got[h])
                worst = max(worst, float(min(np.abs(v - ref).max(), np.abs(v + ref).max())))
                count += 1
    return worst, count, left_out


def motion_error(key):
    """-> (rotation error, translation direction error) in degrees of a job that initialises, None otherwise"""
    r, j = sc.result(*key), sc.job(*key)
    if not r["ok"]:
        return None
    R, t = j["truth"]
    dR = np.asarray(r["R21"], np.float64) @ R.T
    ang = np.degrees(np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1)))
    tt = np.asarray(r["t21"], np.float64)
    dt = np.degrees(np.arccos(np.clip(tt @ t / (np.linalg.norm(tt) * np.linalg.norm(t)), -1, 1)))
    return float(ang), float(dt)


MOTION_KEYS = (sc.MAIN["general"] + (0.0,), sc.MAIN["planar"] + (0.0,))


def motion_spread():
    """-> (largest rotation error, largest translation direction error, jobs that initialise)"""
    errs = [e for e in (motion_error(k) for k in MOTION_KEYS) if e is not None]
    return max(e[0] for e in errs), max(e[1] for e in errs), len(errs)


if __name__ == "__main__":
    w, c, o = null_spread()
    print(f"null vectors compared: {c}\nleft out (s8 > {RATIO} * s7): {o} ({100.0 * o / (c + o):.2f} %)\n"
          f"largest disagreement with float64: {w:.3e}")
    a, b, k = motion_spread()
    print(f"noise-free jobs that initialise: {k} of {len(MOTION_KEYS)}\nlargest rotation error: {a:.3e} degrees\nlargest translation direction error: {b:.3e} degrees")
