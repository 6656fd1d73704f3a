"""Scenes for the PnPsolver tests: a pinhole camera with KITTI intrinsics at a known pose Tcw, points 3 to 9 m in front of it, Gaussian
pixel noise of 0.5 px on the observations, a share of gross outliers (none when n <= 5), octaves spread over 8 levels so that max_err =
sigma2 * 5.991f, and sample rows drawn by the reference's swap-remove procedure (src/PnPsolver.cc:199-212).  Fixed seeds; the model's table
of every job is computed once and shared by the tests that need it."""
import functools

import numpy as np

import pnp_model as pm

f32 = np.float32
K = np.array([718.856, 718.856, 607.1928, 185.2157], f32).astype(np.float64)     # the reference widens the float members of Frame
SF = np.empty(8, f32)
SF[0] = 1.0
for _i in range(1, 8):
    SF[_i] = SF[_i - 1] * f32(1.2)
SIGMA2 = SF * SF
WIDTH, HEIGHT = 1241.0, 376.0


def draw_samples(rng, n, n_hyp):
    """four draws from the indices that are left, the drawn one replaced by the last"""
    out = np.zeros((n_hyp, 4), np.int32)
    for h in range(n_hyp):
        avail = list(range(n))
        for i in range(4):
            r = int(rng.integers(0, len(avail)))
            out[h, i] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return out


def pose(rng):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    ang = rng.uniform(0.1, 0.5)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * (Kx @ Kx)
    return R, rng.uniform(-0.4, 0.4, 3)


@functools.lru_cache(maxsize=None)
def solver(seed, n, n_hyp, outliers=0.3, noise=0.5):
    """-> dict(P3Dw, P2D, sigma2, K, samples, truth=(R, t), is_outlier): what a PnPsolver holds after its constructor"""
    rng = np.random.Generator(np.random.PCG64(seed))
    R, t = pose(rng)
    Xc = np.stack([rng.uniform(-2.5, 2.5, n), rng.uniform(-1.5, 1.5, n), rng.uniform(3.0, 9.0, n)], 1)
    Xw = ((Xc - t) @ R).astype(f32)                     # R^T (Xc - t)
    Xc = Xw.astype(np.float64) @ R.T + t                # what the stored float points project to
    uv = np.stack([K[0] * Xc[:, 0] / Xc[:, 2] + K[2], K[1] * Xc[:, 1] / Xc[:, 2] + K[3]], 1)
    uv += rng.normal(0, 1, (n, 2)) * noise
    out = rng.uniform(size=n) < outliers
    if n <= 5:
        out[:] = False
    uv[out] = np.stack([rng.uniform(0, WIDTH, n), rng.uniform(0, HEIGHT, n)], 1)[out]
    octave = rng.integers(0, 8, n)
    return dict(P3Dw=Xw, P2D=uv.astype(f32), sigma2=SIGMA2[octave], K=K, samples=draw_samples(rng, n, n_hyp), truth=(R, t), is_outlier=out,
                octave=octave)


@functools.lru_cache(maxsize=None)
def job(seed, n, n_hyp, min_inliers, outliers=0.3, noise=0.5):
    """the job of orbx_pnp_hypotheses for that solver"""
    s = solver(seed, n, n_hyp, outliers, noise)
    return dict(s, max_err=pm.max_error(s["sigma2"]), min_inliers=min_inliers)


@functools.lru_cache(maxsize=None)
def table(seed, n, n_hyp, min_inliers):
    return pm.table(job(seed, n, n_hyp, min_inliers))


# (n, n_hyp) of the device tests: n below, at and above one mask word and one reduction stride, n_hyp below and above one workgroup
SHAPES = [(4, 1), (5, 4), (63, 5), (64, 35), (65, 65), (257, 35), (64, 4), (257, 5), (65, 1), (4, 5), (5, 1), (63, 4), (20, 5), (100, 5),
          (64, 5), (257, 1)]


def min_inliers_of(n):
    """half of the correspondences: with 30 % outliers a row sampled from inliers refines and a row that hit an outlier does not"""
    return max(4, n // 2)


def keys():
    return [(200 + i, n, nh, min_inliers_of(n)) for i, (n, nh) in enumerate(SHAPES)]


def batch_keys(size):
    """batches of 1, 3 and 16 jobs that mix n, n_hyp and min_inliers"""
    ks = keys()
    return {1: ks[3:4], 3: [ks[1], ks[12], ks[2]], 16: ks}[size]


# the solvers of the RANSAC tests: (seed, n, rows) with Relocalization's arguments and with a higher epsilon
RANSAC = (301, 100, 90)
RANSAC_PARAMS = (dict(probability=0.99, min_inliers=10, max_iterations=300, min_set=4, epsilon=0.5, th2=5.991),
                 dict(probability=0.99, min_inliers=10, max_iterations=300, min_set=4, epsilon=0.6, th2=5.991))


@functools.lru_cache(maxsize=None)
def special_job():
    """four coplanar samples, two samples with the same 3-D point, a correspondence behind the camera, one with z == 0 at a row's pose,
    and rows that sample them"""
    j = dict(job(7, 40, 8, 12))
    R, t = j["truth"]
    P3, P2 = j["P3Dw"].copy(), j["P2D"].copy()
    # 10 .. 13 on the plane z_c = 5 (coplanar, each with its true projection)
    for k, (x, y) in zip((10, 11, 12, 13), ((-1.0, -0.5), (1.5, -0.75), (1.0, 1.0), (-1.25, 0.5))):
        Xc = np.array([x, y, 5.0])
        P3[k] = ((Xc - t) @ R).astype(f32)
        P2[k] = (K[0] * x / 5.0 + K[2], K[1] * y / 5.0 + K[3])
    P3[15] = P3[14]                                     # the same 3-D point twice
    P3[20] = ((np.array([0.5, 0.25, -4.0]) - t) @ R).astype(f32)   # behind the camera
    good = [int(i) for i in np.nonzero(~j["is_outlier"])[0] if i not in (10, 11, 12, 13, 14, 15, 20, 21)]
    sa = j["samples"].copy()
    sa[1] = (10, 11, 12, 13)
    sa[2] = (14, 15, good[0], good[1])
    sa[3] = (20, good[2], good[3], good[4])
    j.update(P3Dw=P3, P2D=P2)
    # rows 5 and 6: the first two windows of inliers whose four-point pose explains half of the points (four-point EPnP often does not)
    solved = [good[a:a + 4] for a in range(len(good) - 3) if pm.hypothesis(j, good[a:a + 4])[0] >= 20][:2]
    sa[5], sa[6] = solved
    j.update(samples=sa)
    # 21: z == 0 at the pose of row 5, on the plane through the camera centre that row 5's R, t give -- as near as float coordinates
    # come to it: the double expression of the contract is then below 1e-5 (an exact 0.0 is not reachable from float inputs)
    Rm, tm = pm.compute_pose(j, pm.Members(j, sa[5], True))
    P3 = P3.copy()
    P3[21] = ((np.array([0.3, 0.2, 0.0]) - tm) @ Rm).astype(f32)
    j.update(P3Dw=P3, row5_pose=(Rm, tm))
    return j
