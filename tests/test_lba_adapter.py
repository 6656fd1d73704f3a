"""void ORB_SLAM2::Optimizer::LocalBundleAdjustment(KeyFrame*, bool*, Map*) as adapter/lba/LocalBundleAdjustment.cc defines it, compiled
against the stand-in headers of tests/cvstub_lba and run by tests/adapter_lba_driver.cc on a stub map: the keyframe with mnId == 0 among the
local ones, a bad keyframe among the covisible ones and among a point's observers, a bad point, a point that turns bad before the final
loops.  After the call the map holds the poses, the positions and the erased (keyframe, point) pairs, in order, of the direct ABI call on
the problem that the reference's own lists give; UpdateNormalAndDepth ran once per local point; with the flag up nothing was written."""
import os
import subprocess

import numpy as np
import pytest

import lba_scene as ls

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "tests", "adapter_lba_driver.cc"), os.path.join(ROOT, "adapter", "lba", "LocalBundleAdjustment.cc")]
# tests/cvstub_lba in front of tests/cvstub: Optimizer.h, Map.h and the KeyFrame / MapPoint members the existing stand-ins lack
INC = ["-I", os.path.join(ROOT, "adapter", "lba"), "-I", os.path.join(ROOT, "adapter"), "-I", os.path.join(ROOT, "tests", "cvstub_lba"),
       "-I", os.path.join(ROOT, "tests", "cvstub"), "-I", os.path.join(ROOT, "include")]
IDS = [5, 0, 7, 8, 9, 11]        # mnId of the stub keyframes: keyframe 1, a local one, is the map's first
COVIS = [1, 5, 2]                # pKF's covisible keyframes; keyframe 5 is bad
BAD_POINT = 64


def build_driver(tmpdir):
    import __graft_entry__ as ge
    ge.build()
    exe = os.path.join(tmpdir, "adapter_lba_driver")
    pkg_dir = os.path.join(ROOT, "orb-slam2_amd")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"] + INC + SOURCES +
                          ["-L", pkg_dir, "-lorbx", "-lpthread", "-Wl,-rpath," + pkg_dir, "-o", exe])
    return exe


def bits(a):
    return " ".join(f"{v:08x}" for v in np.ascontiguousarray(a, f32).reshape(-1).view(np.uint32))


def stub_map():
    """the stub map of the test from the scene (3, 2, 64, mixed): -> keyframes [dict(id, bad, cam, Tcw, feats [(x, y, ur, isig, point)])], points
    [dict(bad, X)]"""
    pr = ls.shape_scene((3, 2, 64), "mixed")["problem"]
    kfs = [dict(id=IDS[k], bad=0, cam=pr["cam"][k], Tcw=pr["Tcw"][k], feats=[]) for k in range(5)]
    for e in range(len(pr["edge_kf"])):
        kfs[pr["edge_kf"][e]]["feats"].append((pr["x"][e], pr["y"][e], pr["u_right"][e], pr["inv_sigma2"][e], int(pr["edge_point"][e])))
    kfs[0]["feats"].insert(3, (f32(10), f32(20), f32(-1), f32(1), -1))                  # a feature without a point
    kfs[0]["feats"].insert(7, (f32(30), f32(40), f32(-1), f32(1), BAD_POINT))           # a match to a bad point
    kfs.append(dict(id=IDS[5], bad=1, cam=pr["cam"][0], Tcw=pr["Tcw"][0], feats=[(f32(100 + p), f32(90), f32(-1), f32(1), p) for p in range(4)]))
    pts = [dict(bad=0, X=pr["Xw"][p]) for p in range(64)] + [dict(bad=1, X=np.array([1, 2, 3], f32))]
    return kfs, pts


def reference_lists(kfs, pts):
    """src/Optimizer.cc:530-734 on the stub map -> the problem of the ABI call, the keyframe and point lists, (keyframe, point) of every edge"""
    local = [0] + [k for k in COVIS if not kfs[k]["bad"]]
    marked = set([0] + COVIS)
    lpts = []
    for k in local:
        for (_, _, _, _, p) in kfs[k]["feats"]:
            if p >= 0 and not pts[p]["bad"] and p not in lpts:
                lpts.append(p)
    obs = {p: sorted((k, i) for k in range(len(kfs)) for i, ft in enumerate(kfs[k]["feats"]) if ft[4] == p) for p in lpts}    # pointer order
    fixed = []
    for p in lpts:
        for k, _ in obs[p]:
            if k not in marked:
                marked.add(k)
                if not kfs[k]["bad"]:
                    fixed.append(k)
    order = local + fixed
    ek, ep, x, y, ur, isig, pairs = [], [], [], [], [], [], []
    for ip, p in enumerate(lpts):
        for k, i in obs[p]:
            if kfs[k]["bad"]:
                continue
            ft = kfs[k]["feats"][i]
            ek.append(order.index(k)); ep.append(ip); x.append(ft[0]); y.append(ft[1]); ur.append(ft[2]); isig.append(ft[3]); pairs.append((k, p))
    problem = dict(Tcw=np.stack([kfs[k]["Tcw"] for k in order]), cam=np.stack([kfs[k]["cam"] for k in order]),
                   fixed=np.array([kfs[k]["id"] == 0 for k in local] + [1] * len(fixed), np.uint8), Xw=np.stack([pts[p]["X"] for p in lpts]),
                   edge_kf=np.array(ek, np.int32), edge_point=np.array(ep, np.int32), x=np.array(x, f32), y=np.array(y, f32),
                   u_right=np.array(ur, f32), inv_sigma2=np.array(isig, f32))
    return problem, local, fixed, lpts, pairs


def write_scene(path, kfs, pts, stop, turns_bad):
    with open(path, "w") as f:
        f.write(f"{int(stop)}\n{len(kfs)} {len(pts)}\n")
        for K in kfs:
            f.write(f"{K['id']} {K['bad']} {bits(K['cam'])}\n{bits(K['Tcw'])}\n{len(K['feats'])}\n")
            for (x, y, ur, isig, p) in K["feats"]:
                f.write(f"{bits([x, y, ur, isig])} {p}\n")
        f.write(f"{len(COVIS)} " + " ".join(str(k) for k in COVIS) + "\n")
        for j, P in enumerate(pts):
            f.write(f"{P['bad']} {int(j == turns_bad)} {bits(P['X'])}\n")


def run_driver(exe, path):
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0 and "adaptor lba ok" in r.stdout, r.stdout + r.stderr
    kf, pt, erased = {}, {}, []
    un = lambda words: np.array([int(v, 16) for v in words], np.uint32).view(f32)
    for ln in r.stdout.splitlines():
        w = ln.split()
        if w[0] == "kf":
            kf[int(w[1])] = (int(w[3]), int(w[5]), un(w[7:]).reshape(4, 4))
        elif w[0] == "pt":
            pt[int(w[1])] = (int(w[3]), int(w[5]), un(w[7:]))
        elif w[0] == "erased":
            erased.append((int(w[1]), int(w[2])))
    return kf, pt, erased


def test_driver_compiles_without_warnings(tmp_path):
    exe = build_driver(str(tmp_path))
    assert subprocess.run([exe], capture_output=True).returncode == 2       # usage


@pytest.mark.gpu
def test_adaptor_equals_the_abi_call(pkg, tmp_path):
    exe = build_driver(str(tmp_path))
    kfs, pts = stub_map()
    problem, local, fixed, lpts, pairs = reference_lists(kfs, pts)
    assert local == [0, 1, 2] and sorted(fixed) == [3, 4] and list(problem["fixed"]) == [0, 1, 0, 1, 1] and BAD_POINT not in lpts and len(lpts) >= 60
    assert lpts != sorted(lpts)                                             # the points go up in the lists' order, not the map's
    exp = pkg.local_bundle_adjustment(problem)
    assert exp["stopped"] == 0 and exp["n_erase"] > 4
    mono = problem["u_right"] < 0
    erase = (exp["edge_flags"] & 2) != 0
    turns_bad = pairs[int(np.nonzero(erase)[0][1])][1]                      # a point with an edge in vToErase turns bad during the call
    want = [pairs[e] for m in (True, False) for e in range(len(pairs)) if mono[e] == m and erase[e] and pairs[e][1] != turns_bad]
    assert mono[erase].any() and not mono[erase].all() and len(want) < exp["n_erase"]
    path = str(tmp_path / "scene.txt")
    write_scene(path, kfs, pts, 0, turns_bad)
    kf, pt, erased = run_driver(exe, path)
    assert erased == want
    order = local + fixed
    for k in range(len(kfs)):
        calls, erase_calls, T = kf[k]
        if k in local:
            assert calls == 1 and T.tobytes() == exp["Tcw"][order.index(k)].tobytes(), k
        else:
            assert calls == 0 and T.tobytes() == np.asarray(kfs[k]["Tcw"], f32).tobytes(), k
        assert erase_calls == sum(1 for (kk, _) in want if kk == k)
    for j in range(len(pts)):
        sets, updates, X = pt[j]
        if j in lpts:                                                       # the point that turned bad included (:854-861)
            assert (sets, updates) == (1, 1) and X.tobytes() == exp["Xw"][lpts.index(j)].tobytes(), j
        else:
            assert (sets, updates) == (0, 0) and X.tobytes() == np.asarray(pts[j]["X"], f32).tobytes(), j
    # with the flag up nothing is written
    write_scene(path, kfs, pts, 1, turns_bad)
    kf, pt, erased = run_driver(exe, path)
    assert erased == [] and all(v[0] == 0 and v[1] == 0 for v in kf.values()) and all(v[0] == 0 and v[1] == 0 for v in pt.values())
    assert all(kf[k][2].tobytes() == np.asarray(kfs[k]["Tcw"], f32).tobytes() for k in range(len(kfs)))
