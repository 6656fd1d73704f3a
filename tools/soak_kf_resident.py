"""Randomized parity soak of the resident-keyframe searches (include/orbx.h: orbx_frame_window_best, _window_best_batch, _search_by_sim3,
_search_by_projection_sim3): random scenes of tests/test_projection.py, random job mixes in one batch launch (keyframes named twice,
empty jobs, keyframes without features), resident == host-pointer twin == CPU oracle.
Run on the GPU box: python tools/soak_kf_resident.py [seconds] [seed]"""
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
FR = ("x", "y", "octave", "angle", "u_right", "desc", "bounds")


def cut(d, n):
    return {k: (v[:n] if isinstance(v, np.ndarray) else v) for k, v in d.items()}


t0 = time.time(); trial = 0; searches = 0; jobs_run = 0; found = 0
mt = pkg.ORBmatcher(0.9, True)
while time.time() - t0 < budget:
    trial += 1
    # a handful of keyframes of random size (now and then none or one feature, or more than the grid's LDS path holds) with their points
    scenes = []
    for k in range(int(rng.integers(1, 5))):
        nc = int(rng.choice([0, 1])) if rng.random() < 0.1 else int(rng.integers(8193, 11000)) if rng.random() < 0.05 else int(rng.integers(2, 2500))
        npnt = int(rng.integers(1, 2500))
        cur, pts, sf = TP._scene(70000 + 10 * trial + k, max(nc, 2), npnt, dense=bool(rng.random() < 0.4), stereo_frac=float(rng.choice([0, 0.5, 1])))
        cur = cut(cur, nc)
        p2 = dict(pts); p2["aux"] = (pts["u"] - float(rng.choice([0.0, 5.0, 8.0]))).astype(f32)
        scenes.append((pkg.DeviceFrame({k_: cur[k_] for k_ in FR}), cur, p2, sf, (1.0 / (sf * sf)).astype(f32)))
    tag = f"trial {trial}"
    spec = []
    for j in range(int(rng.integers(1, 9))):
        kf, cur, p2, sf, inv = scenes[int(rng.integers(0, len(scenes)))]
        n = len(p2["u"])
        p = cut(p2, int(rng.choice([0, 1, 3, n])) if rng.random() < 0.3 else int(rng.integers(0, n + 1)))
        spec.append((kf, cur, p, sf, inv, float(rng.choice([1.0, 3.0, 4.0, 7.5, 12.0, 40.0])), int(rng.integers(0, 2)), int(rng.choice([0, 30, 50, 100, 255]))))   # (at 256 the oracle also counts a point whose window holds only inadmissible candidates)
    res = mt.FuseResidentBatch([dict(kf=kf, points=p, scaleFactors=sf, invLevelSigma2=inv if chi2 else None, th=th, max_dist=md)
                                for kf, cur, p, sf, inv, th, chi2, md in spec])
    for (kf, cur, p, sf, inv, th, chi2, md), (bi, bd, n) in zip(spec, res):
        ebi, ebd, en = O.window_best(cur, p, sf, inv, th, chi2, md) if len(p["u"]) and kf.n else (np.full(len(p["u"]), -1), np.full(len(p["u"]), 256), 0)
        assert n == en and (bi == ebi).all() and (bd == ebd).all(), f"batch {tag} nc {kf.n} np {len(p['u'])} th {th} chi2 {chi2} md {md}"
        sbi, sbd, sn = mt.FuseResident(kf, p, sf, inv if chi2 else None, th, md)
        hbi, hbd, hn = mt.Fuse(cur, p, sf, inv if chi2 else None, th, md)
        assert sn == hn == en and (sbi == ebi).all() and (hbi == ebi).all() and (sbd == ebd).all() and (hbd == ebd).all(), f"single {tag} nc {kf.n} np {len(p['u'])}"
        jobs_run += 1; found += n
    # the Sim3 projection search with a random vpMatched, and SearchBySim3 on a pair of keyframes
    kf, cur, p2, sf, inv = scenes[0]
    occ = (rng.random(kf.n) < float(rng.choice([0, 0.1, 0.5]))).astype(np.uint8)
    th = float(rng.choice([3.0, 10.0]))
    g, n = mt.SearchByProjectionSim3Resident(kf, occ, p2, sf, th); e, en = O.search_by_projection_sim3(dict(cur, occupied=occ), p2, sf, th)
    assert n == en and (g == e).all(), "sim3 projection " + tag
    ns = int(rng.integers(2, 1500))
    c1, c2, p12, p21, sf = TP._sim3_scene(90000 + trial, ns)
    k1, k2 = pkg.DeviceFrame({k_: c1[k_] for k_ in FR}), pkg.DeviceFrame({k_: c2[k_] for k_ in FR})
    g, n = mt.SearchBySim3Resident(k1, k2, p12, p21, sf, sf, 7.5); e, en = O.search_by_sim3(c1, c2, p12, p21, sf, sf, 7.5)
    h, hn = mt.SearchBySim3(c1, c2, p12, p21, sf, sf, 7.5)
    assert n == en == hn and (g == e).all() and (h == e).all(), "sim3 " + tag
    searches += 2
    if trial % 20 == 0: print(f"{time.time() - t0:6.1f}s trials {trial}", flush=True)
print(f"resident-keyframe soak done: {trial} random job mixes, {jobs_run} window_best jobs (batch == single == host-pointer twin == oracle, "
      f"{found} points found), {searches} Sim3 searches, every one equal to the oracle")
