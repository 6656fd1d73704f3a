"""orbx_adapter::RefreshMapPoints (adapter/mappoint/MapPointRefresh.cc), compiled with -Werror against the stand-ins of
tests/cvstub_refresh and run by tests/adapter_refresh_driver.cc.  The driver's keyframes lie in one array, so the order of their addresses
-- the reference's order over a point's observations -- is the order of their slots, the device call's: the adaptor must leave every
MapPoint member byte-equal to the reference's two functions run point by point.  Covered: the geometry on the device with the descriptors
on the host while no keyframe is resident, all three forms with resident keyframes, bad keyframes whose observations linger, reference
keyframes outside the row, a point at a camera centre, a point the graph does not know (the host fallback), a hole and a repeat in the
list, and the real orbx_adapter::LocalMapPoints behind the hooks it announces itself with: a SearchLocalPoints fills the table, the
members change on the host, RefreshMapPoints writes the table in place, every slot then holds its point's members and the next
SearchLocalPoints has nothing to send, while a change the refresh did not make is still sent."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "tests", "adapter_refresh_driver.cc"), os.path.join(ROOT, "adapter", "mappoint", "MapPointRefresh.cc"),
           os.path.join(ROOT, "adapter", "mapgraph", "MapGraph.cc"), os.path.join(ROOT, "adapter", "localmap", "LocalMapPoints.cc")]
INC = ["-I", os.path.join(ROOT, "adapter", "mappoint"), "-I", os.path.join(ROOT, "adapter", "mapgraph"), "-I", os.path.join(ROOT, "adapter", "localmap"),
       "-I", os.path.join(ROOT, "adapter"),
       "-I", os.path.join(ROOT, "tests", "cvstub_refresh"), "-I", os.path.join(ROOT, "tests", "cvstub"), "-I", os.path.join(ROOT, "include")]
CXX = ["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror"]
ENV = dict(os.environ, ORBX_MAPGRAPH_KEYFRAMES="64", ORBX_MAPGRAPH_FEATURES="64", ORBX_MAPGRAPH_POINTS="4096", ORBX_MAPGRAPH_OBS="16", ORBX_MAPPOINTS_CAPACITY="512")


def build_driver(tmpdir):
    import __graft_entry__ as ge
    ge.build()
    exe = os.path.join(tmpdir, "adapter_refresh_driver")
    pkg_dir = os.path.join(ROOT, "orb-slam2_amd")
    subprocess.check_call(CXX + ["-O2"] + INC + SOURCES + ["-L", pkg_dir, "-lorbx", "-lpthread", "-Wl,-rpath," + pkg_dir, "-o", exe])
    return exe


def test_driver_compiles_without_warnings(tmp_path):
    exe = build_driver(str(tmp_path))
    assert subprocess.run([exe], capture_output=True).returncode == 2       # usage


def test_hook_owners_compile_without_warnings():
    """the two files that register themselves with the refresh adaptor, against their own stand-ins"""
    a = os.path.join(ROOT, "adapter")
    for src, stubs in ((os.path.join(a, "localmap", "LocalMapPoints.cc"), ["cvstub_localmap", "cvstub"]), (os.path.join(a, "ORBmatcher_batch.cc"), ["cvstub"])):
        inc = ["-I", os.path.dirname(src), "-I", a] + [x for s in stubs for x in ("-I", os.path.join(ROOT, "tests", s))] + ["-I", os.path.join(ROOT, "include")]
        subprocess.check_call(CXX + ["-fsyntax-only"] + inc + [src])


@pytest.mark.gpu
def test_members_equal_the_reference_functions(tmp_path):
    exe = build_driver(str(tmp_path))
    r = subprocess.run([exe, "check"], capture_output=True, text=True, env=ENV)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "adaptor refresh ok" in r.stdout
    assert r.stdout.count("points updated") == 6      # no frames, the three forms, bad keyframes, with the table
