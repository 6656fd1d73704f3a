"""int ORB_SLAM2::Optimizer::PoseOptimization(Frame *pFrame) as adapter/pose/PoseOptimization.cc defines it, compiled against the stand-in
headers of tests/cvstub_pose and run by tests/adapter_pose_driver.cc on a stub Frame with monocular and stereo features and NULL points:
mvbOutlier, the return value and the pose equal the direct ABI call on the same values; with fewer than 3 points SetPose is not called."""
import os
import subprocess

import numpy as np
import pytest

import pose_scene as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "tests", "adapter_pose_driver.cc"), os.path.join(ROOT, "adapter", "pose", "PoseOptimization.cc")]
# tests/cvstub_pose in front of tests/cvstub: Optimizer.h, and the Frame / MapPoint members the existing stand-ins lack
INC = ["-I", os.path.join(ROOT, "adapter", "pose"), "-I", os.path.join(ROOT, "adapter"), "-I", os.path.join(ROOT, "tests", "cvstub_pose"),
       "-I", os.path.join(ROOT, "tests", "cvstub"), "-I", os.path.join(ROOT, "include")]


def build_driver(tmpdir):
    import __graft_entry__ as ge
    ge.build()
    exe = os.path.join(tmpdir, "adapter_pose_driver")
    pkg_dir = os.path.join(ROOT, "orb-slam2_amd")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"] + INC + SOURCES +
                          ["-L", pkg_dir, "-lorbx", "-lpthread", "-Wl,-rpath," + pkg_dir, "-o", exe])
    return exe


def bits(a):
    return " ".join(f"{v:08x}" for v in np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32))


def write_scene(path, sc):
    o = sc["obs"]
    with open(path, "w") as f:
        f.write(bits(sc["cam"]) + "\n" + bits(sc["Tcw"]) + "\n" + str(len(o["x"])) + "\n")
        for i in range(len(o["x"])):
            f.write(f"{int(o['has_point'][i])} " + bits([o["x"][i], o["y"][i], o["u_right"][i], o["inv_sigma2"][i], *o["Xw"][i]]) + "\n")


def run_driver(exe, path):
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0 and "adaptor pose ok" in r.stdout, r.stdout + r.stderr
    out = dict(ln.split(" ", 1) for ln in r.stdout.splitlines() if " " in ln)
    T = np.array([int(v, 16) for v in out["Tcw"].split()], np.uint32).view(np.float32).reshape(4, 4)
    return int(out["ret"]), int(out["setpose"]), T, np.array([int(c) for c in out["outlier"].strip()], np.uint8)


def test_driver_compiles_without_warnings(tmp_path):
    exe = build_driver(str(tmp_path))
    assert subprocess.run([exe], capture_output=True).returncode == 2       # usage


@pytest.mark.gpu
@pytest.mark.parametrize("n,mix", [(65, "mixed"), (2, "mixed")])
def test_adaptor_equals_the_abi_call(pkg, tmp_path, n, mix):
    exe = build_driver(str(tmp_path))
    sc = ps.scene(ps.seed_of(n, mix), n, mix)
    path = str(tmp_path / "scene.txt")
    write_scene(path, sc)
    ret, setpose, T, outlier = run_driver(exe, path)
    exp = pkg.pose_optimize(sc["obs"], sc["cam"], sc["Tcw"])
    has = sc["obs"]["has_point"].astype(bool)
    assert ret == exp["n_inliers"] and T.tobytes() == exp["Tcw"].tobytes()
    assert (outlier[has] == exp["outlier"][has]).all() and (outlier[~has] == 1).all()      # the flags of features without a point stay
    if n >= 3:
        assert setpose == 1 and ret > 0 and exp["outlier"][has].any() and sc["stereo"][has].any() and not sc["stereo"][has].all()
    else:
        assert setpose == 0 and ret == 0 and T.tobytes() == sc["Tcw"].tobytes() and not outlier[has].any()
