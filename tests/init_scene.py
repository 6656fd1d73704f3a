"""Scenes for the Initializer tests: synthetic two-view scenes with K = (500, 500, 320, 240), the keypoints rounded to float, the matches
scattered among unmatched keypoints of both frames (Normalize runs over all of them), sample rows drawn by the reference's swap-remove
procedure.  Fixed seeds; the model's table and result of every job are computed once and shared by the tests that need them.

  general      a depth-varied cloud seen under a sideways translation: F must win
  planar       one plane: H must win
  no_parallax  a pure rotation: Initialize must return false
  outliers     general with 25 % of the matches replaced by random pairs

n takes {8, 63, 64, 65, 130, 257} (below, at and above one mask word and two), n_hyp {1, 5, 64, 65, 200} (below, at and above a workgroup
of four waves per model)."""
import functools

import numpy as np

import init_model as im

f32 = np.float32
K = np.array([500.0, 500.0, 320.0, 240.0], f32)
SCENES = ("general", "planar", "no_parallax", "outliers")
KEYS = (("general", 257, 200), ("general", 130, 64), ("general", 65, 65), ("general", 64, 5), ("general", 63, 1), ("general", 8, 5),
        ("planar", 257, 200), ("planar", 130, 65), ("planar", 64, 64), ("planar", 8, 1),
        ("no_parallax", 257, 64), ("no_parallax", 63, 5),
        ("outliers", 257, 200), ("outliers", 130, 64), ("outliers", 65, 5))
MAIN = {"general": ("general", 257, 200), "planar": ("planar", 257, 200), "no_parallax": ("no_parallax", 257, 64),
        "outliers": ("outliers", 257, 200)}


def keys():
    return list(KEYS)


def draw_samples(rng, n, n_hyp):
    """:95-111: eight draws from the indices that are left, the drawn one replaced by the last"""
    out = np.zeros((n_hyp, 8), np.int32)
    for h in range(n_hyp):
        avail = list(range(n))
        for i in range(8):
            r = int(rng.integers(0, len(avail)))
            out[h, i] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return out


def rotation(axis, ang):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * (Kx @ Kx)


def project(X):
    return np.stack([K[0] * X[:, 0] / X[:, 2] + K[2], K[1] * X[:, 1] / X[:, 2] + K[3]], 1)


@functools.lru_cache(maxsize=None)
def job(kind, n, n_hyp, noise=0.3):
    """-> the job dict of init_model plus truth = (R, t) with x2 ~ R X1 + t, X = the points in camera 1, is_outlier[n]"""
    seed = 1000 * SCENES.index(kind) + n + 7 * n_hyp
    rng = np.random.Generator(np.random.PCG64(seed))
    X = np.stack([rng.uniform(-2.5, 2.5, n), rng.uniform(-1.8, 1.8, n), rng.uniform(4.0, 10.0, n)], 1)
    if kind == "planar":
        X[:, 2] = 6.0 + 1.2 * X[:, 0] + 0.3 * X[:, 1]   # tilted: the twin solution of the plane loses its points
    R = rotation(rng.normal(size=3), 0.06)
    t = np.zeros(3) if kind == "no_parallax" else np.array([0.6, 0.05, 0.03])
    p1 = project(X) + rng.normal(0, noise, (n, 2))
    p2 = project(X @ R.T + t) + rng.normal(0, noise, (n, 2))
    out = np.zeros(n, bool)
    if kind == "outliers":
        out = rng.uniform(size=n) < 0.25
        p2[out] = np.stack([rng.uniform(0, 640, n), rng.uniform(0, 480, n)], 1)[out]
    n1, n2 = n + 5 + n // 7, n + 3 + n // 5
    xy1 = np.stack([rng.uniform(0, 640, n1), rng.uniform(0, 480, n1)], 1)
    xy2 = np.stack([rng.uniform(0, 640, n2), rng.uniform(0, 480, n2)], 1)
    first = np.sort(rng.choice(n1, n, replace=False))
    second = rng.choice(n2, n, replace=False)
    xy1[first] = p1
    xy2[second] = p2
    return dict(xy1=xy1.astype(f32), xy2=xy2.astype(f32), matches=np.stack([first, second], 1).astype(np.int32), K=K, sigma=1.0,
                min_parallax=1.0, min_triangulated=50, samples=draw_samples(rng, n, n_hyp), truth=(R, t), X=X, is_outlier=out)


@functools.lru_cache(maxsize=None)
def table(kind, n, n_hyp, noise=0.3):
    """the model's table of a job; shared, never written"""
    return im.table(job(kind, n, n_hyp, noise))


@functools.lru_cache(maxsize=None)
def result(kind, n, n_hyp, noise=0.3):
    """the model's Initialize of a job; shared, never written"""
    return im.initialize(job(kind, n, n_hyp, noise), table(kind, n, n_hyp, noise))


@functools.lru_cache(maxsize=None)
def degenerate_job():
    """Points 4 and 5 of the contract in one job of 40 matches.  Every coordinate of frame 2 is a multiple of 1/4 and the keypoints lie in
    pairs P + d, P - d around P = (320, 240), so Normalize's float sums are exact and its mean IS P.  The eight matches of sample row 0
    all sit at P in frame 2: their normalised (u2, v2) are exactly (0, 0), columns 6-8 of the 16 x 9 system and columns 0-5 of the 8 x 9
    system are exactly zero, the null vector is a unit vector, H21i has two zero columns, H12i = inv(H21i) is the ZERO matrix, chiSquare1
    is NaN for every match and the score is NaN while the first gate stays open.  Fpre has one non-zero entry: two singular values are
    exactly zero and their columns of U stay zero.  Row 1 is an ordinary row."""
    rng = np.random.Generator(np.random.PCG64(77))
    n, n1, n2 = 40, 52, 48
    P = np.array([320.0, 240.0])
    d = np.round(rng.uniform(-150, 150, ((n2 - 8) // 2, 2)) * 4) / 4
    xy2 = np.concatenate([np.tile(P, (8, 1)), P + d, P - d]).astype(f32)
    xy1 = np.stack([rng.uniform(0, 640, n1), rng.uniform(0, 480, n1)], 1).astype(f32)
    first = np.sort(rng.choice(n1, n, replace=False))
    second = np.concatenate([np.arange(8), 8 + rng.choice(n2 - 8, n - 8, replace=False)])
    sa = np.stack([np.arange(8), 8 + draw_samples(rng, n - 8, 1)[0]]).astype(np.int32)
    return dict(xy1=xy1, xy2=xy2, matches=np.stack([first, second], 1).astype(np.int32), K=K, sigma=1.0, min_parallax=1.0,
                min_triangulated=50, samples=sa)


@functools.lru_cache(maxsize=None)
def scoreless_job():
    """a job in which no hypothesis scores above 0: sigma so small that every match fails every gate of every model"""
    j = dict(job("outliers", 65, 5))
    j.update(sigma=1e-4)
    return j
