"""orbx_adapter::CreateNewMapPointsBatch (adapter/triangulate/CreateNewMapPoints.cc) compiled against the stand-in headers of
tests/cvstub_triangulate (in front of tests/cvstub: the KeyFrame members mvKeys, mvDepth, mb, invfx, invfy) and run by
tests/adapter_triangulate_driver.cc on a stub map of 1 + 3 keyframes, unregistered and registered with KeyFrameFrames: `out` equals the
ABI call on the captured inputs in creation order, no feature of the current keyframe gets two points, and the resident call gives the
same bits."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "tests", "adapter_triangulate_driver.cc"), os.path.join(ROOT, "adapter", "triangulate", "CreateNewMapPoints.cc"),
           os.path.join(ROOT, "adapter", "ORBmatcher_batch.cc")]
INC = ["-I", os.path.join(ROOT, "adapter", "triangulate"), "-I", os.path.join(ROOT, "adapter"), "-I", os.path.join(ROOT, "tests", "cvstub_triangulate"),
       "-I", os.path.join(ROOT, "tests", "cvstub"), "-I", os.path.join(ROOT, "include")]


def build_driver(tmpdir):
    import __graft_entry__ as ge
    ge.build()
    exe = os.path.join(tmpdir, "adapter_triangulate_driver")
    pkg_dir = os.path.join(ROOT, "orb-slam2_amd")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-Werror", "-DORBX_ADAPTER_CAPTURE"] + INC + SOURCES +
                          ["-L", pkg_dir, "-lorbx", "-lpthread", "-Wl,-rpath," + pkg_dir, "-o", exe])
    return exe


def test_driver_compiles_without_warnings(tmp_path):
    exe = build_driver(str(tmp_path))
    assert subprocess.run([exe], capture_output=True).returncode == 2       # usage
    # a production build (no capture) compiles too
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-Werror", "-c"] + INC + [SOURCES[1], "-o", str(tmp_path / "plain.o")])


@pytest.mark.gpu
def test_adaptor_equals_the_abi_call(pkg, tmp_path):
    exe = build_driver(str(tmp_path))
    r = subprocess.run([exe, "check"], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and "adaptor triangulate ok" in r.stdout, r.stdout + r.stderr
