"""ORB_SLAM2::Optimizer::OptimizeEssentialGraph as adapter/essential/OptimizeEssentialGraph.cc defines it, compiled against the stand-in
headers of tests/cvstub_eg (Map, KeyFrame, MapPoint, LoopClosing::KeyFrameAndPose, Optimizer.h) in front of tests/cvstub_sim3opt (the
g2o::Sim3 stand-in) and tests/cvstub, and run by tests/adapter_eg_driver.cc on a stub map: pLoopKF is not first; one bad keyframe is
another's parent and someone's covisible (the stated deviation: no vertex, its edges skipped); a covisibility pair is already in
sInsertedEdges; one weight is 99 and one is 100; the pCurKF-pLoopKF connection is below minFeat and is kept anyway (:971); a loop edge to a
larger mnId is skipped (:1039); one point has mnCorrectedByKF == pCurKF->mnId; one point is bad and one hangs on the bad keyframe.  After
the call the map holds what the direct ABI call on the reference's own lists returns, bit for bit, every SetPose was made under
mMutexMapUpdate, and UpdateNormalAndDepth was called once per good point.  The declaration is the reference's
(tools/gen_optimizeessentialgraph_interface.py)."""
import os
import subprocess

import numpy as np
import pytest

import eg_scene as es

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "tests", "adapter_eg_driver.cc"), os.path.join(ROOT, "adapter", "essential", "OptimizeEssentialGraph.cc")]
INC = ["-I", os.path.join(ROOT, "adapter", "essential"), "-I", os.path.join(ROOT, "adapter"), "-I", os.path.join(ROOT, "tests", "cvstub_eg"),
       "-I", os.path.join(ROOT, "tests", "cvstub_sim3opt"), "-I", os.path.join(ROOT, "tests", "cvstub"), "-I", os.path.join(ROOT, "include")]
MIN_FEAT = 100
# the stub keyframes in the map's order: the scene keyframe each carries (None: the bad one).  mnId = 10 x the scene index; the bad one 15.
STUB = [1, 0, None, 2, 3, 4, 5, 6, 7, 8]
BAD, LOOP, CUR = 2, 1, 9


def build_driver(tmpdir):
    import __graft_entry__ as ge
    ge.build()
    exe = os.path.join(tmpdir, "adapter_eg_driver")
    pkg_dir = os.path.join(ROOT, "orb-slam2_amd")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"] + INC + SOURCES +
                          ["-L", pkg_dir, "-lorbx", "-lpthread", "-Wl,-rpath," + pkg_dir, "-o", exe])
    return exe


def bits(a):
    return " ".join(f"{v:08x}" for v in np.ascontiguousarray(a, f32).reshape(-1).view(np.uint32))


def bits64(a):
    return " ".join(f"{v:016x}" for v in np.ascontiguousarray(a, np.float64).reshape(-1).view(np.uint64))


def stub_map():
    """-> keyframes [dict(id, bad, parent, Tcw, corrected, noncorrected, loop [indices], cov [(index, weight)])], connections {index: [indices]},
    points [dict(bad, by, cref, ref, X)]"""
    pr = es.make(8, 0, 9911)
    of = {s: k for k, s in enumerate(STUB) if s is not None}                  # scene keyframe -> stub index
    kfs = []
    for s in STUB:
        if s is None:
            kfs.append(dict(id=15, bad=1, Tcw=pr["Tcw"][1], corrected=None, noncorrected=None))
        else:
            c, n = pr["corrected"][s], pr["noncorrected"][s]
            kfs.append(dict(id=10 * s, bad=0, Tcw=pr["Tcw"][s], corrected=pr["S_corrected"][c] if c >= 0 else None,
                            noncorrected=pr["S_noncorrected"][n] if n >= 0 else None))
    parents = {1: 0, 2: None, 3: 2, 4: 3, 5: 2, 6: 5, 7: 6, 8: 7}              # scene keyframe 2 hangs on the bad one; 5 is not on the chain
    for k, K in enumerate(kfs):
        K["parent"], K["loop"], K["cov"] = -1, [], []
    for s, p in parents.items():
        kfs[of[s]]["parent"] = BAD if p is None else of[p]
    kfs[BAD]["parent"] = of[1]
    kfs[of[5]]["loop"] = [of[1]]                                               # an earlier loop: an edge at keyframe 5 ...
    kfs[of[1]]["loop"] = [of[5]]                                               # ... and none at keyframe 1 (:1039)
    cov = {3: [(of[2], 150), (of[1], 120), (BAD, 110)],                        # its parent; an edge; the bad keyframe
           4: [(of[2], 100), (of[1], 99)],                                     # 100 is an edge, 99 is not
           6: [(of[4], 130), (of[3], 105)],
           7: [(of[8], 200), (of[1], 120), (of[5], 115)],                      # its child; a pair already in sInsertedEdges; an edge
           8: [(of[7], 200), (of[6], 101), (of[0], 50)],                       # its parent; an edge; the loop keyframe below minFeat
           2: [(of[3], 150), (of[4], 100)]}                                    # its child; a larger mnId
    for s, lst in cov.items():
        kfs[of[s]]["cov"] = lst
    connections = {of[7]: [of[1]], of[8]: [of[1], of[0]]}                      # (8, 1) has no weight: dropped; (8, 0) is kept by :971
    pts = []
    for p in range(len(pr["Xw"])):
        pts.append(dict(bad=0, by=0, cref=0, ref=of[int(pr["point_ref"][p])], X=pr["Xw"][p]))
    pts[3].update(by=80, cref=30, ref=of[5])                                   # corrected by pCurKF: nIDr = mnCorrectedReference
    pts[4]["bad"] = 1
    pts[5]["ref"] = BAD                                                        # no vertex for its reference keyframe: left alone
    pts[6].update(by=70, cref=30)                                              # corrected by another keyframe: GetReferenceKeyFrame
    return kfs, connections, pts, int(pr["fix_scale"])


def reference_lists(kfs, connections, pts):
    """src/Optimizer.cc:914-1138 on the stub map, with the stated deviation -> the problem of the ABI call, the keyframe and point lists"""
    order = [k for k in range(len(kfs)) if not kfs[k]["bad"]]
    vertex = {k: i for i, k in enumerate(order)}
    by_id = {kfs[k]["id"]: vertex[k] for k in order}
    weight = lambda a, b: dict(kfs[a]["cov"]).get(b, 0)
    children = lambda a: [k for k in range(len(kfs)) if kfs[k]["parent"] == a]
    ei, ej, kind, inserted = [], [], [], set()

    def add(a, b, kd):
        if a in vertex and b in vertex:
            ei.append(vertex[a]); ej.append(vertex[b]); kind.append(kd)
    for a in sorted(connections):
        for b in sorted(connections[a]):
            if (kfs[a]["id"] != kfs[CUR]["id"] or kfs[b]["id"] != kfs[LOOP]["id"]) and weight(a, b) < MIN_FEAT:
                continue
            add(a, b, 0)
            inserted.add((min(kfs[a]["id"], kfs[b]["id"]), max(kfs[a]["id"], kfs[b]["id"])))
    for a in order:
        K = kfs[a]
        if K["parent"] >= 0:
            add(a, K["parent"], 1)
        for b in sorted(K["loop"]):
            if kfs[b]["id"] < K["id"]:
                add(a, b, 1)
        for b, w in K["cov"]:
            if w < MIN_FEAT or b == K["parent"] or b in children(a) or b in K["loop"] or kfs[b]["bad"] or not kfs[b]["id"] < K["id"]:
                continue
            if (min(K["id"], kfs[b]["id"]), max(K["id"], kfs[b]["id"])) in inserted:
                continue
            add(a, b, 1)
    corrected, noncorrected, Sc, Sn = [], [], [], []
    for k in order:
        for key, idx, arr in (("corrected", corrected, Sc), ("noncorrected", noncorrected, Sn)):
            if kfs[k][key] is None:
                idx.append(-1)
            else:
                idx.append(len(arr)); arr.append(kfs[k][key])
    lpts, ref = [], []
    for j, P in enumerate(pts):
        if P["bad"]:
            continue
        nid = P["cref"] if P["by"] == kfs[CUR]["id"] else kfs[P["ref"]]["id"]
        if nid in by_id:
            lpts.append(j); ref.append(by_id[nid])
    problem = dict(Tcw=np.stack([kfs[k]["Tcw"] for k in order]), fixed=np.array([k == LOOP for k in order], np.uint8),
                   corrected=np.array(corrected, np.int32), noncorrected=np.array(noncorrected, np.int32),
                   S_corrected=np.array(Sc).reshape(-1, 8), S_noncorrected=np.array(Sn).reshape(-1, 8),
                   edge_i=np.array(ei, np.int32), edge_j=np.array(ej, np.int32), edge_kind=np.array(kind, np.uint8),
                   Xw=np.stack([pts[j]["X"] for j in lpts]), point_ref=np.array(ref, np.int32), fix_scale=0)
    return problem, order, lpts


def write_scene(path, kfs, connections, pts, fix_scale):
    with open(path, "w") as f:
        f.write(f"{fix_scale} {LOOP} {CUR} {len(kfs)} {len(pts)} {len(connections)}\n")
        for K in kfs:
            f.write(f"{K['id']} {K['bad']} {K['parent']}\n{bits(K['Tcw'])}\n")
            for key in ("corrected", "noncorrected"):
                f.write(f"{key} 0\n" if K[key] is None else f"{key} 1 {bits64(K[key])}\n")
            f.write(f"{len(K['loop'])} {' '.join(str(b) for b in K['loop'])}\n")
            f.write(f"{len(K['cov'])} {' '.join(f'{b} {w}' for b, w in K['cov'])}\n")
        for a in sorted(connections):
            f.write(f"{a} {len(connections[a])} {' '.join(str(b) for b in connections[a])}\n")
        for P in pts:
            f.write(f"{P['bad']} {P['by']} {P['cref']} {P['ref']} {bits(P['X'])}\n")


def run_driver(exe, path):
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0 and "adaptor eg ok" in r.stdout, r.stdout + r.stderr
    un = lambda words: np.array([int(v, 16) for v in words], np.uint32).view(f32)
    kf, pt = {}, {}
    for ln in r.stdout.splitlines():
        w = ln.split()
        if w[0] == "kf":
            kf[int(w[1])] = dict(setpose=int(w[3]), unlocked=int(w[5]), Tcw=un(w[7:]).reshape(4, 4))
        elif w[0] == "pt":
            pt[int(w[1])] = dict(set=int(w[3]), update=int(w[5]), pos=un(w[7:]))
    return kf, pt


def test_driver_compiles_without_warnings(tmp_path):
    exe = build_driver(str(tmp_path))
    assert subprocess.run([exe], capture_output=True).returncode == 2       # usage


def test_reference_lists_of_the_stub_map():
    kfs, connections, pts, fix = stub_map()
    problem, order, lpts = reference_lists(kfs, connections, pts)
    assert order == [0, 1, 3, 4, 5, 6, 7, 8, 9] and problem["fixed"].tolist() == [0, 1, 0, 0, 0, 0, 0, 0, 0]
    v = {s: order.index(k) for k, s in enumerate(STUB) if s is not None}       # scene keyframe -> vertex
    edges = list(zip(problem["edge_i"].tolist(), problem["edge_j"].tolist(), problem["edge_kind"].tolist()))
    assert edges[:2] == [(v[7], v[1], 0), (v[8], v[0], 0)]                     # (8, 1) dropped by its weight, (8, 0) kept below minFeat
    assert (v[2], v[1], 1) not in edges and all(v[2] != i for i, j, k in edges if k == 1 and j == v[1])   # keyframe 2's parent is bad
    assert (v[5], v[1], 1) in edges and (v[1], v[5], 1) not in edges           # the loop edge once, at the larger mnId
    assert (v[3], v[1], 1) in edges and (v[4], v[2], 1) in edges and (v[4], v[1], 1) not in edges    # 120, 100, 99
    assert (v[7], v[1], 1) not in edges and (v[7], v[5], 1) in edges and (v[8], v[6], 1) in edges    # sInsertedEdges
    assert (v[8], v[0], 1) not in edges and (v[2], v[4], 1) not in edges
    assert 4 not in lpts and 5 not in lpts and problem["point_ref"][lpts.index(3)] == v[3] and problem["point_ref"][lpts.index(6)] != v[3]


@pytest.mark.gpu
def test_adaptor_equals_the_abi_call(pkg, tmp_path):
    exe = build_driver(str(tmp_path))
    kfs, connections, pts, fix = stub_map()
    problem, order, lpts = reference_lists(kfs, connections, pts)
    exp = pkg.optimize_essential_graph(problem)
    assert exp["iterations"] >= 1 and exp["chi2"] < exp["chi2_start"]
    path = str(tmp_path / "scene.txt")
    write_scene(path, kfs, connections, pts, fix)
    kf, pt = run_driver(exe, path)
    for k in range(len(kfs)):
        if k in order:
            assert kf[k]["setpose"] == 1 and kf[k]["unlocked"] == 0 and kf[k]["Tcw"].tobytes() == exp["Tcw"][order.index(k)].tobytes(), k
        else:
            assert kf[k]["setpose"] == 0 and kf[k]["Tcw"].tobytes() == np.asarray(kfs[k]["Tcw"], f32).tobytes(), k
    for j in range(len(pts)):
        if j in lpts:
            assert (pt[j]["set"], pt[j]["update"]) == (1, 1) and pt[j]["pos"].tobytes() == exp["Xw"][lpts.index(j)].tobytes(), j
        else:
            assert (pt[j]["set"], pt[j]["update"]) == (0, 0) and pt[j]["pos"].tobytes() == np.asarray(pts[j]["X"], f32).tobytes(), j
    assert any(not np.array_equal(kf[k]["Tcw"], np.asarray(kfs[k]["Tcw"], f32)) for k in order)


def test_declaration_is_the_reference_s():
    """the stand-in header and the adaptor's definition against tests/golden/reference_optimizeessentialgraph_interface.json, and the
    fixture against the reference's own include/Optimizer.h where the checkout is present"""
    import json
    from tools import gen_optimizeessentialgraph_interface as gi
    fix = json.load(open(gi.FIXTURE))
    assert gi.decl(open(os.path.join(ROOT, "tests", "cvstub_eg", "Optimizer.h")).read()) == fix
    own = gi.decl(open(SOURCES[1]).read(), qualified=True)
    assert own["return"] == fix["return"] and own["params"] == fix["params"]
    ref = os.path.join(os.path.dirname(gi.rf.gsf.REF), "include", "Optimizer.h")
    if os.path.exists(ref):
        assert gi.decl(open(ref, errors="replace").read()) == fix
