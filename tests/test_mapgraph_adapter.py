"""orbx_adapter::MapGraph, LocalMapping::KeyFrameCulling, CovisibilityCounts and VoteLocalKeyFrames as adapter/mapgraph/MapGraph.cc defines
them, compiled with -Werror against the stand-ins of tests/cvstub_graph (whose mutators are the reference's and fire the hooks) and run by
tests/adapter_mapgraph_driver.cc: a stub map built through the mutators only -- with the keyframe of mnId 0 among the covisibles, an
mbNotErase keyframe, observations without a match and matches without an observation, a repeated AddObservation, and keyframes and points
made at the addresses of objects that went away without a word -- is culled by the adaptor and, on a copy, by a plain host loop; bad
keyframes, bad points, every mvpMapPoints and every mObservations must be the same, again after fusions, erasures, a new keyframe and a
second culling, and the two vote functions must fill the reference's maps as the host loops do.
Without a GPU the same driver runs against a host stand-in of the ABI (tests/mapgraph_abi_stub.cc) under the address and
undefined-behaviour sanitizers: that run checks the adaptor's host bookkeeping -- slots, queue, echoes."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "tests", "adapter_mapgraph_driver.cc"), os.path.join(ROOT, "adapter", "mapgraph", "MapGraph.cc")]
STUB = os.path.join(ROOT, "tests", "mapgraph_abi_stub.cc")
INC = ["-I", os.path.join(ROOT, "adapter", "mapgraph"), "-I", os.path.join(ROOT, "adapter"), "-I", os.path.join(ROOT, "tests", "cvstub_graph"),
       "-I", os.path.join(ROOT, "tests", "cvstub"), "-I", os.path.join(ROOT, "include")]
CXX = ["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror"]
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
# a graph sized for the stub map, not for a session
ENV = dict(os.environ, ORBX_MAPGRAPH_KEYFRAMES="64", ORBX_MAPGRAPH_FEATURES="64", ORBX_MAPGRAPH_POINTS="4096", ORBX_MAPGRAPH_OBS="16")


def build_driver(tmpdir):
    import __graft_entry__ as ge
    ge.build()
    exe = os.path.join(tmpdir, "adapter_mapgraph_driver")
    pkg_dir = os.path.join(ROOT, "orb-slam2_amd")
    subprocess.check_call(CXX + ["-O2"] + INC + SOURCES + ["-L", pkg_dir, "-lorbx", "-lpthread", "-Wl,-rpath," + pkg_dir, "-o", exe])
    return exe


def check_output(r):
    assert r.returncode == 0, r.stdout + r.stderr
    rounds = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("round ")]
    assert len(rounds) == 2 and int(rounds[0][3]) >= 1, r.stdout              # something was culled
    assert int(rounds[0][7]) >= 1                                            # and a point went bad with it
    assert int(rounds[1][13]) > int(rounds[0][13]) > 0                       # hook calls were recognised as already applied, both times
    assert int(rounds[1][11]) < 400, r.stdout                                # about 1 400 hook calls travel as batches, not one by one
    assert "adaptor mapgraph ok" in r.stdout


def test_driver_compiles_without_warnings(tmp_path):
    exe = build_driver(str(tmp_path))
    assert subprocess.run([exe], capture_output=True).returncode == 2       # usage


@pytest.mark.parametrize("mode", ["stereo", "mono"])
def test_host_bookkeeping_under_sanitizers(tmp_path, mode):
    exe = os.path.join(str(tmp_path), "adapter_mapgraph_driver_san")
    probe = os.path.join(str(tmp_path), "probe.cc")
    open(probe, "w").write("int main() { return 0; }\n")
    have = subprocess.run(["g++"] + SANITIZE + [probe, "-o", exe], capture_output=True).returncode == 0 and subprocess.run([exe]).returncode == 0
    subprocess.check_call(CXX + (SANITIZE if have else ["-O1"]) + INC + SOURCES + [STUB, "-lpthread", "-o", exe])
    r = subprocess.run([exe, "check"] + (["mono"] if mode == "mono" else []), capture_output=True, text=True, env=ENV)
    check_output(r)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["stereo", "mono"])
def test_culling_equals_the_host_loop(tmp_path, mode):
    exe = build_driver(str(tmp_path))
    r = subprocess.run([exe, "check"] + (["mono"] if mode == "mono" else []), capture_output=True, text=True, env=ENV)
    check_output(r)
