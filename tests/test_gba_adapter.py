"""ORB_SLAM2::Optimizer::GlobalBundleAdjustemnt / BundleAdjustment as adapter/ba/BundleAdjustment.cc defines them, compiled against the
stand-in headers of tests/cvstub_gba and run by tests/adapter_gba_driver.cc on a stub map: the keyframe with mnId == 0 not first, a bad
keyframe, a bad point, a point all of whose observers are bad, a point that turns bad before the recovery, a good observer that the map's
list does not hold (the stated deviation: its observations are skipped) and one newer than maxKFid.  After the call the map holds what the
direct ABI call on the problem the reference's own lists give returns: with nLoopKF == 0 through SetPose / SetWorldPos /
UpdateNormalAndDepth, otherwise in mTcwGBA / mPosGBA / mnBAGlobalForKF with none of the three called."""
import os
import subprocess

import numpy as np
import pytest

import lba_scene as ls

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "tests", "adapter_gba_driver.cc"), os.path.join(ROOT, "adapter", "ba", "BundleAdjustment.cc")]
# tests/cvstub_gba in front of tests/cvstub_lba and tests/cvstub: Map::GetAllKeyFrames / GetAllMapPoints and the GBA members
INC = ["-I", os.path.join(ROOT, "adapter", "ba"), "-I", os.path.join(ROOT, "adapter"), "-I", os.path.join(ROOT, "tests", "cvstub_gba"),
       "-I", os.path.join(ROOT, "tests", "cvstub_lba"), "-I", os.path.join(ROOT, "tests", "cvstub"), "-I", os.path.join(ROOT, "include")]
# the stub keyframes: (mnId, bad, in the map's list, the scene keyframe whose pose and observations it carries)
STUB = [(5, 0, 1, 0), (7, 1, 1, None), (0, 0, 1, 3), (8, 0, 1, 1), (9, 0, 1, 2), (3, 0, 0, None), (20, 0, 0, None)]
BAD_POINT, ORPHAN, TURNS_BAD = 64, 65, 10
ITERATIONS = 6


def build_driver(tmpdir):
    import __graft_entry__ as ge
    ge.build()
    exe = os.path.join(tmpdir, "adapter_gba_driver")
    pkg_dir = os.path.join(ROOT, "orb-slam2_amd")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"] + INC + SOURCES +
                          ["-L", pkg_dir, "-lorbx", "-lpthread", "-Wl,-rpath," + pkg_dir, "-o", exe])
    return exe


def bits(a):
    return " ".join(f"{v:08x}" for v in np.ascontiguousarray(a, f32).reshape(-1).view(np.uint32))


def stub_map():
    """-> keyframes [dict(id, bad, in_map, cam, Tcw, feats [(x, y, ur, isig, point)])], points [dict(bad, X)]"""
    pr = ls.scene(7411, 3, 1, 64, "mixed")["problem"]
    assert pr["fixed"].tolist() == [0, 0, 0, 1]
    kfs = []
    for (mnid, bad, in_map, src) in STUB:
        s = 0 if src is None else src
        kfs.append(dict(id=mnid, bad=bad, in_map=in_map, cam=pr["cam"][s], Tcw=pr["Tcw"][s], feats=[]))
    of_scene = {src: k for k, (_, _, _, src) in enumerate(STUB) if src is not None}
    for e in range(len(pr["edge_kf"])):
        kfs[of_scene[int(pr["edge_kf"][e])]]["feats"].append((pr["x"][e], pr["y"][e], pr["u_right"][e], pr["inv_sigma2"][e], int(pr["edge_point"][e])))
    kfs[0]["feats"].insert(3, (f32(10), f32(20), f32(-1), f32(1), -1))                  # a feature without a point
    kfs[0]["feats"].insert(7, (f32(30), f32(40), f32(-1), f32(1), BAD_POINT))           # an observation of a bad point
    kfs[1]["feats"] = [(f32(100 + p), f32(90), f32(-1), f32(1), p) for p in (0, 1, 2, ORPHAN)]      # the bad keyframe: ORPHAN's only observer
    kfs[5]["feats"] = [(f32(200 + p), f32(80), f32(-1), f32(1), p) for p in (3, 4, 5)]              # not in the list, mnId <= maxKFid
    kfs[6]["feats"] = [(f32(300 + p), f32(70), f32(-1), f32(1), p) for p in (5, 6)]                 # not in the list, mnId > maxKFid
    pts = [dict(bad=0, X=pr["Xw"][p]) for p in range(64)] + [dict(bad=1, X=np.array([1, 2, 3], f32)), dict(bad=0, X=np.array([.1, .2, .3], f32))]
    return kfs, pts


def reference_lists(kfs, pts):
    """src/Optimizer.cc:85-224 on the stub map -> the problem of the ABI call, the keyframe and point lists"""
    order = [k for k in range(len(kfs)) if kfs[k]["in_map"] and not kfs[k]["bad"]]
    max_id = max(kfs[k]["id"] for k in order)
    lpts = [p for p in range(len(pts)) if not pts[p]["bad"]]
    ek, ep, x, y, ur, isig = [], [], [], [], [], []
    for ip, p in enumerate(lpts):
        for k in range(len(kfs)):                                                       # pointer order
            for ft in kfs[k]["feats"]:
                if ft[4] != p or kfs[k]["bad"] or kfs[k]["id"] > max_id:
                    continue
                if k not in order:                                                      # the stated deviation
                    continue
                ek.append(order.index(k)); ep.append(ip); x.append(ft[0]); y.append(ft[1]); ur.append(ft[2]); isig.append(ft[3])
    problem = dict(Tcw=np.stack([kfs[k]["Tcw"] for k in order]), cam=np.stack([kfs[k]["cam"] for k in order]),
                   fixed=np.array([kfs[k]["id"] == 0 for k in order], np.uint8), Xw=np.stack([pts[p]["X"] for p in lpts]),
                   edge_kf=np.array(ek, np.int32), edge_point=np.array(ep, np.int32), x=np.array(x, f32), y=np.array(y, f32),
                   u_right=np.array(ur, f32), inv_sigma2=np.array(isig, f32))
    return problem, order, lpts


def write_scene(path, kfs, pts, stop, loop_kf, robust):
    with open(path, "w") as f:
        f.write(f"{int(stop)} {loop_kf} {ITERATIONS} {int(robust)}\n{len(kfs)} {len(pts)}\n")
        for K in kfs:
            f.write(f"{K['id']} {K['bad']} {K['in_map']} {bits(K['cam'])}\n{bits(K['Tcw'])}\n{len(K['feats'])}\n")
            for (x, y, ur, isig, p) in K["feats"]:
                f.write(f"{bits([x, y, ur, isig])} {p}\n")
        for j, P in enumerate(pts):
            f.write(f"{P['bad']} {int(j == TURNS_BAD)} {bits(P['X'])}\n")


def run_driver(exe, path):
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0 and "adaptor gba ok" in r.stdout, r.stdout + r.stderr
    un = lambda words: None if words == ["-"] else np.array([int(v, 16) for v in words], np.uint32).view(f32)
    kf, pt = {}, {}
    for ln in r.stdout.splitlines():
        w = ln.split()
        if w[0] == "kf":
            g = w.index("gba")
            kf[int(w[1])] = dict(setpose=int(w[3]), mark=int(w[5]), Tcw=un(w[7:g]).reshape(4, 4), gba=un(w[g + 1:]))
        elif w[0] == "pt":
            g = w.index("gba")
            pt[int(w[1])] = dict(set=int(w[3]), update=int(w[5]), mark=int(w[7]), pos=un(w[9:g]), gba=un(w[g + 1:]))
    return kf, pt


def test_driver_compiles_without_warnings(tmp_path):
    exe = build_driver(str(tmp_path))
    assert subprocess.run([exe], capture_output=True).returncode == 2       # usage


@pytest.mark.gpu
def test_adaptor_equals_the_abi_call(pkg, tmp_path):
    exe = build_driver(str(tmp_path))
    kfs, pts = stub_map()
    problem, order, lpts = reference_lists(kfs, pts)
    assert order == [0, 2, 3, 4] and problem["fixed"].tolist() == [0, 1, 0, 0] and BAD_POINT not in lpts and ORPHAN in lpts
    path = str(tmp_path / "scene.txt")
    for loop_kf, robust in ((0, True), (7, False)):
        exp = pkg.bundle_adjustment(problem, iterations=ITERATIONS, robust=robust)
        assert exp["stopped"] == 0 and exp["trials"] >= 2 and exp["n_active_kf"] == 3
        assert exp["point_included"][lpts.index(ORPHAN)] == 0 and exp["point_included"].sum() == len(lpts) - 1
        write_scene(path, kfs, pts, 0, loop_kf, robust)
        kf, pt = run_driver(exe, path)
        for k in range(len(kfs)):
            got, start = kf[k], np.asarray(kfs[k]["Tcw"], f32)
            if k in order and loop_kf == 0:
                assert got["setpose"] == 1 and got["Tcw"].tobytes() == exp["Tcw"][order.index(k)].tobytes(), k
                assert got["mark"] == 0 and got["gba"] is None
            elif k in order:
                assert got["setpose"] == 0 and got["Tcw"].tobytes() == start.tobytes(), k
                assert got["mark"] == loop_kf and got["gba"].tobytes() == exp["Tcw"][order.index(k)].tobytes(), k
            else:
                assert got["setpose"] == 0 and got["mark"] == 0 and got["gba"] is None and got["Tcw"].tobytes() == start.tobytes(), k
        for j in range(len(pts)):
            got, start = pt[j], np.asarray(pts[j]["X"], f32)
            written = j in lpts and j not in (ORPHAN, TURNS_BAD)
            if written and loop_kf == 0:
                assert (got["set"], got["update"], got["mark"]) == (1, 1, 0) and got["gba"] is None
                assert got["pos"].tobytes() == exp["Xw"][lpts.index(j)].tobytes(), j
            elif written:
                assert (got["set"], got["update"], got["mark"]) == (0, 0, loop_kf) and got["pos"].tobytes() == start.tobytes()
                assert got["gba"].tobytes() == exp["Xw"][lpts.index(j)].tobytes(), j
            else:                                                               # bad, without an edge, or bad by the recovery: nothing
                assert (got["set"], got["update"], got["mark"]) == (0, 0, 0) and got["gba"] is None and got["pos"].tobytes() == start.tobytes(), j
    # the flag up at the call: no iteration, and the recovery still runs (the start estimates through the quaternion round trip)
    exp = pkg.bundle_adjustment(problem, iterations=0)
    write_scene(path, kfs, pts, 1, 0, True)
    kf, pt = run_driver(exe, path)
    assert all(kf[k]["setpose"] == 1 and kf[k]["Tcw"].tobytes() == exp["Tcw"][order.index(k)].tobytes() for k in order)
    assert all(pt[j]["pos"].tobytes() == np.asarray(pts[j]["X"], f32).tobytes() for j in range(len(pts)))
