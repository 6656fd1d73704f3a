"""Randomized parity soak of the resident-frame searches (include/orbx.h: orbx_frame_search_by_projection_*) against the CPU oracle:
random scenes of tests/test_projection.py, one DeviceFrame per scene searched several times with changing `occupied`, thresholds and
directions.  Run on the GPU box: python tools/soak_frame_resident.py [seconds] [seed]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import __graft_entry__ as ge
from oracle import oracle_py as O
import test_projection as TP
pkg = ge.load_pkg()
budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
rng = np.random.Generator(np.random.PCG64(int(sys.argv[2]) if len(sys.argv) > 2 else 7))
f32 = np.float32
t0 = time.time(); trial = 0; searches = 0
while time.time() - t0 < budget:
    trial += 1
    nc = int(rng.integers(1, 2500)) if trial % 10 else int(rng.integers(8193, 12000)); npnt = int(rng.integers(1, 2500)); dense = bool(trial % 3 == 0)
    cur, pts, sf = TP._scene(50000 + trial, nc, npnt, dense=dense, stereo_frac=float(rng.choice([0, 0.5, 1])),
                             obs_frac=float(rng.choice([0, 0.3, 0.7, 1])), occ_frac=float(rng.choice([0, 0.1, 0.5])))
    df = pkg.DeviceFrame({k: cur[k] for k in ("x", "y", "octave", "angle", "u_right", "desc", "bounds")})
    tag = f"trial {trial} nc {nc} np {npnt} dense {dense}"
    for rep in range(3):
        occ = (rng.random(nc) < float(rng.choice([0, 0.1, 0.5]))).astype(np.uint8)
        c = dict(cur, occupied=occ)
        th = float(rng.choice([1.0, 3.0, 7.0, 15.0, 40.0])); co = int(rng.choice([0, 1, 3])); ratio = float(rng.choice([0.6, 0.8, 0.9]))
        m = pkg.ORBmatcher(ratio, co != 0)
        d = int(rng.integers(0, 3))
        g, n = m.SearchByProjectionLastFrameResident(df, occ, pts, sf, th, d, 40.0, check_orientation=co)
        e, en = O.search_by_projection_last(c, pts, sf, th, d, 40.0, co)
        assert n == en and (g == e).all(), "last " + tag
        p2 = dict(pts); p2["aux"] = (pts["u"] - 5).astype(f32)
        g, n = m.SearchByProjectionMapPointsResident(df, occ, p2, sf, th); e, en = O.search_by_projection_points(c, p2, sf, th, ratio)
        assert n == en and (g == e).all(), "points " + tag
        od = int(rng.choice([50, 64, 100]))
        g, n = m.SearchByProjectionKeyFrameResident(df, occ, pts, sf, th, od, check_orientation=co)
        e, en = O.search_by_projection_keyframe(c, pts, sf, th, od, co)
        assert n == en and (g == e).all(), "kf " + tag
        searches += 3
    if trial % 50 == 0: print(f"{time.time() - t0:6.1f}s trials {trial}", flush=True)
print(f"resident-frame soak done: {trial} random scenes, {searches} resident searches, every one equal to the oracle")
