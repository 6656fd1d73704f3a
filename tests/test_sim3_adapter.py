"""ORB_SLAM2::Sim3Solver and orbx_adapter::Sim3SolverBatch (adapter/sim3/Sim3Solver.cc) compiled against the stand-in headers of
tests/cvstub_sim3 (in front of tests/cvstub: KeyFrame::mK and a seeded DUtils::Random) and run by tests/adapter_sim3_driver.cc on a stub
map of one current keyframe and three loop candidates: the gather against the driver's own loop, the batch against solvers evaluated one
by one on the same random stream, and both against a replay of the ABI call's table on the captured inputs.  The adaptor's public
interface is held to the reference's by tests/golden/reference_sim3solver_interface.json (tools/gen_sim3_interface.py)."""
import json
import os
import subprocess

import pytest

from tools import gen_sim3_interface as gi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
SOURCES = [os.path.join(ROOT, "tests", "adapter_sim3_driver.cc"), os.path.join(ROOT, "adapter", "sim3", "Sim3Solver.cc")]
INC = ["-I", os.path.join(ROOT, "adapter", "sim3"), "-I", os.path.join(ROOT, "adapter"), "-I", os.path.join(ROOT, "tests", "cvstub_sim3"),
       "-I", os.path.join(ROOT, "tests", "cvstub"), "-I", os.path.join(ROOT, "include")]


def build_driver(tmpdir):
    import __graft_entry__ as ge
    ge.build()
    exe = os.path.join(tmpdir, "adapter_sim3_driver")
    pkg_dir = os.path.join(ROOT, "orb-slam2_amd")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-Werror", "-DORBX_ADAPTER_CAPTURE"] + INC + SOURCES +
                          ["-L", pkg_dir, "-lorbx", "-lpthread", "-Wl,-rpath," + pkg_dir, "-o", exe])
    return exe


def test_driver_compiles_without_warnings(tmp_path):
    exe = build_driver(str(tmp_path))
    assert subprocess.run([exe], capture_output=True).returncode == 2       # usage
    # a production build (no capture) compiles too
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-Werror", "-c"] + INC + [SOURCES[1], "-o", str(tmp_path / "plain.o")])


def test_public_interface_is_the_reference_headers():
    """every public member of the reference's include/Sim3Solver.h, with its return and parameter types, in the adaptor's header; and
    the size_t element type of mvnMaxError1/2 that the contract's truncated thresholds rest on.  Where the reference checkout is present
    the record is re-derived from its header first"""
    fix = json.load(open(gi.FIXTURE))
    assert len(fix["public"]) == 7 and fix["max_error"] == {"mvnMaxError1": "size_t", "mvnMaxError2": "size_t"}
    hdr = os.path.join(REF, "include", "Sim3Solver.h")
    if os.path.exists(hdr):
        assert gi.sim3solver_interface(open(hdr, errors="replace").read()) == fix, "the recorded interface is not the reference header's"
    mine = gi.sim3solver_interface(open(os.path.join(ROOT, "adapter", "sim3", "Sim3Solver.h")).read())
    assert mine["public"] == fix["public"]


@pytest.mark.gpu
def test_adaptor_equals_the_abi_call(pkg, tmp_path):
    exe = build_driver(str(tmp_path))
    r = subprocess.run([exe, "check"], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and "adaptor sim3 ok" in r.stdout, r.stdout + r.stderr
