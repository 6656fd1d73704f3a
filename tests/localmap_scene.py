"""Scenes for the resident map-point tests: a camera, a pose, a frame of features and a local map whose points project onto them.
Shared by tests/test_mappoints.py and tests/test_local_points.py; the expected values come from tests/frustum_model.py."""
import numpy as np

from tools import synth

f32 = np.float32
W, H = 640, 480
CAM = np.array([500.0, 500.0, 320.0, 240.0, 40.0, 0.0, 0.0, W, H], f32)        # fx fy cx cy mbf mnMinX mnMinY mnMaxX mnMaxY
EDGE_CAM = np.array([512.0, 512.0, 0.0, 0.0, 40.0, 0.0, 0.0, W, H], f32)       # u = 512 * X / Z exactly: bounds can be hit to the bit
IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0], f32)        # Rcw tcw Ow
LSF = f32(np.log(f32(1.2)))
NLEVELS = 8
SF = np.array([f32(1.2) ** i for i in range(NLEVELS)], f32)


def pose(seed):
    """a small rotation and a translation: Rcw[9] tcw[3] Ow[3] with Ow = -Rcw^T tcw in float"""
    rng = np.random.Generator(np.random.PCG64(seed))
    a = rng.normal(0, 0.08, 3)
    th = np.linalg.norm(a); k = a / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = (np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K).astype(f32)
    t = rng.normal(0, 0.3, 3).astype(f32)
    Ow = (-(R.T.astype(np.float64) @ t.astype(np.float64))).astype(f32)
    return np.concatenate([R.reshape(9), t, Ow]).astype(f32)


def scene(seed, n_feat=200, n_pts=300, cluster=0):
    """-> frame (dict for DeviceFrame, with `occupied`), geom[n_pts][8], desc[n_pts][32], has_obs[n_pts], pose.  Most points are the
    back-projection of a feature (so that the search finds matches); `cluster` further points crowd round one feature with confusable
    descriptors (the claim order by has_obs then decides who keeps it); some points lie behind the camera, outside the image, outside
    their distance range or face away."""
    rng = np.random.Generator(np.random.PCG64(seed))
    po = pose(seed)
    R = po[:9].reshape(3, 3).astype(np.float64); t = po[9:12].astype(np.float64); Ow = po[12:15].astype(np.float64)
    x = rng.uniform(5, W - 5, n_feat).astype(f32); y = rng.uniform(5, H - 5, n_feat).astype(f32)
    octave = rng.integers(0, NLEVELS, n_feat).astype(np.int32)
    fdesc = rng.integers(0, 256, (n_feat, 32), dtype=np.uint8)
    src = rng.integers(0, n_feat, n_pts)
    if cluster:
        src[:cluster] = src[0]
        near = np.argsort((x - x[src[0]]) ** 2 + (y - y[src[0]]) ** 2)[:8]      # the features round the cluster look alike
        fdesc[near] = synth.flip_bits(rng, np.repeat(fdesc[src[0]][None], len(near), 0), 0.04)
    z = rng.uniform(2.0, 8.0, n_pts)
    u = x[src] + rng.normal(0, 1.2, n_pts); v = y[src] + rng.normal(0, 1.2, n_pts)
    pc = np.stack([(u - CAM[2]) / CAM[0] * z, (v - CAM[3]) / CAM[1] * z, z], 1)
    pw = (pc - t) @ R                                                            # R^T (pc - t)
    bad = rng.random(n_pts)
    if cluster:
        bad[:cluster] = 1.0
    pw[bad < 0.04] = Ow + (pw[bad < 0.04] - Ow) * -1.0                           # behind the camera
    pw[(bad >= 0.04) & (bad < 0.08), 0] += 30.0                                  # outside the image
    d = np.linalg.norm(pw - Ow, axis=1)
    normal = (pw - Ow) / d[:, None] + rng.normal(0, 0.15, (n_pts, 3))
    normal /= np.linalg.norm(normal, axis=1)[:, None]
    normal[(bad >= 0.08) & (bad < 0.12)] *= -1.0                                 # faces away
    lvl = octave[src]
    dmax = d * (1.2 ** lvl) * rng.uniform(0.93, 0.99, n_pts)                     # PredictScale lands on the feature's octave, mostly
    dmin = dmax / 1.2 ** (NLEVELS - 1)
    far = (bad >= 0.12) & (bad < 0.15)
    dmax[far] = d[far] * 0.5; dmin[far] = dmax[far] * 0.1                        # beyond 1.2 * dmax
    geom = np.concatenate([pw, dmin[:, None], normal, dmax[:, None]], 1).astype(f32)
    desc = synth.flip_bits(rng, fdesc[src], 0.05)
    u_right = np.where(rng.random(n_feat) < 0.5, x - 40.0 / rng.uniform(2.0, 8.0, n_feat), -1).astype(f32)
    frame = dict(x=x, y=y, octave=octave, angle=rng.uniform(0, 360, n_feat).astype(f32), u_right=u_right, desc=fdesc,
                 occupied=(rng.random(n_feat) < 0.1).astype(np.uint8), bounds=(0.0, 0.0, float(W), float(H)))
    has_obs = (rng.random(n_pts) < 0.7).astype(np.uint8)
    return frame, geom, desc, has_obs, po
