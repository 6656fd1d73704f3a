"""Scenes for the Sim3Solver tests: two cameras with different intrinsics that see the same points, related by a known similarity
X1 = s R X2 + t (s != 1, or s = 1 for fix_scale), Gaussian noise of pixel size on the points of camera 1, a share of gross outliers,
octaves spread over 8 levels with the truncated thresholds of the contract, and sample rows drawn by the reference's swap-remove
procedure.  Fixed seeds; the model's table of every job is computed once and shared by the tests that need it."""
import functools

import numpy as np

import sim3_model as sm

f32 = np.float32
K1 = np.array([718.856, 718.856, 607.1928, 185.2157], f32)
K2 = np.array([535.4, 539.2, 320.1, 247.6], f32)
SF = np.empty(8, f32)
SF[0] = 1.0
for _i in range(1, 8):
    SF[_i] = SF[_i - 1] * f32(1.2)
SIGMA2 = SF * SF


def draw_samples(rng, n, n_hyp):
    """:166-181: three draws from the indices that are left, the drawn one replaced by the last"""
    out = np.zeros((n_hyp, 3), np.int32)
    for h in range(n_hyp):
        avail = list(range(n))
        for i in range(3):
            r = int(rng.integers(0, len(avail)))
            out[h, i] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return out


def similarity(rng, fix_scale):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    ang = rng.uniform(0.1, 0.5)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * (Kx @ Kx)
    s = 1.0 if fix_scale else float(rng.uniform(0.7, 1.4))
    t = rng.uniform(-0.4, 0.4, 3)
    return s, R, t


@functools.lru_cache(maxsize=None)
def job(seed, n, n_hyp, fix_scale, outliers=0.3, noise=0.5):
    """-> dict(X1, X2, max_err1, max_err2, K1, K2, fix_scale, samples, truth=(s, R, t), clean=X1 without noise, is_outlier)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    s, R, t = similarity(rng, fix_scale)
    X2 = np.stack([rng.uniform(-2.5, 2.5, n), rng.uniform(-1.5, 1.5, n), rng.uniform(3.0, 9.0, n)], 1)
    clean = s * (X2 @ R.T) + t
    X1 = clean.copy()
    X1[:, 0] += rng.normal(0, noise, n) * X1[:, 2] / K1[0]
    X1[:, 1] += rng.normal(0, noise, n) * X1[:, 2] / K1[1]
    X1[:, 2] += rng.normal(0, noise, n) * X1[:, 2] * X1[:, 2] / (K1[0] * 0.5)   # depth from a 0.5 m baseline
    out = rng.uniform(size=n) < outliers
    if n <= 3:
        out[:] = False
    X1[out] = np.stack([rng.uniform(-2.5, 2.5, n), rng.uniform(-1.5, 1.5, n), rng.uniform(3.0, 9.0, n)], 1)[out]
    o1, o2 = rng.integers(0, 8, n), rng.integers(0, 8, n)
    thr = np.array([sm.threshold(v) for v in SIGMA2], f32)
    return dict(X1=X1.astype(f32), X2=X2.astype(f32), max_err1=thr[o1], max_err2=thr[o2], K1=K1, K2=K2, fix_scale=bool(fix_scale),
                samples=draw_samples(rng, n, n_hyp), truth=(s, R, t), clean=clean.astype(f32), is_outlier=out, octave1=o1, octave2=o2)


@functools.lru_cache(maxsize=None)
def table(seed, n, n_hyp, fix_scale):
    return sm.table(job(seed, n, n_hyp, fix_scale))


# (n, n_hyp) of the device tests: below, at and above one mask word and one workgroup of four waves
SHAPES = [(3, 1), (20, 5), (63, 63), (64, 64), (65, 65), (257, 300), (64, 1), (20, 65), (65, 5), (257, 63)]


def keys():
    """the jobs of the suite: every shape with both fix_scale values"""
    return [(100 + i, n, nh, bool((i + k) & 1)) for k in range(2) for i, (n, nh) in enumerate(SHAPES) if k == 0 or i < 6]


def batch_keys(size):
    """batches of 1, 3 and 16 jobs that mix the shapes and both fix_scale values"""
    ks = keys()
    return {1: ks[5:6], 3: [ks[1], ks[12], ks[4]], 16: ks}[size]


def special_job():
    """three coincident correspondences (a degenerate hypothesis), a point behind camera 1, a point with z == 0 in camera 2, and rows
    that sample them"""
    j = dict(job(7, 40, 8, False))
    X1, X2 = j["X1"].copy(), j["X2"].copy()
    X1[[11, 12]] = X1[10]
    X2[[11, 12]] = X2[10]
    X1[20, 2] = -X1[20, 2]
    X2[21, 2] = 0.0
    sa = j["samples"].copy()
    sa[1] = (10, 11, 12)
    sa[2] = (12, 10, 11)
    sa[3] = (20, 5, 6)
    sa[4] = (7, 21, 8)
    good = [int(i) for i in np.nonzero(~j["is_outlier"])[0] if i not in (10, 11, 12, 20, 21)]
    sa[5], sa[6] = good[0:3], good[3:6]        # rows with inliers, so that the two special points are tested against a real solution
    j.update(X1=X1, X2=X2, samples=sa)
    return j
