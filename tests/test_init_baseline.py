"""tools/init_baseline.cc, the plain C++ loop that tools/bench_init.py times beside the device call, against tests/init_model.py: the same
scores, matrices and mask words.  A second, compiled statement of the contract of include/orbx.h that needs no GPU -- and the check that
the bench tool's host figure is the figure of the same arithmetic."""
import ctypes as C
import os
import subprocess

import pytest

import init_model as im
import init_scene as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def baseline(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("init_baseline") / "libinit_baseline.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC",
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "init_baseline.cc"), "-o", so])
    return C.CDLL(so)


def test_plain_loop_equals_the_model(pkg, baseline):
    ox = pkg.orbx
    baseline.mono_init_table_loop.argtypes = [C.POINTER(ox.MonoInitJob)]
    for key in sc.keys():
        J, keep, out = ox._mono_init_job(sc.job(*key), "t")
        assert baseline.mono_init_table_loop(C.byref(J)) == 0
        assert all(a.tobytes() == b.tobytes() for a, b in zip(out, sc.table(*key))), key
    j = sc.degenerate_job()                                  # the zero inverse, the NaN score, the zero singular values
    J, keep, out = ox._mono_init_job(j, "t")
    assert baseline.mono_init_table_loop(C.byref(J)) == 0
    assert all(a.tobytes() == b.tobytes() for a, b in zip(out, im.table(j)))
