"""tools/pnp_baseline.cc, the plain C++ loop that tools/bench_pnp.py times beside the device call, against tests/pnp_model.py: the same
counts, masks and pose bits.  A second, compiled statement of the contract of include/orbx.h that needs no GPU -- and the check that the
bench tool's host figure is the figure of the same arithmetic."""
import ctypes as C
import os
import subprocess

import pytest

import pnp_scene as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def baseline(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("pnp_baseline") / "libpnp_baseline.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC",
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "pnp_baseline.cc"), "-o", so])
    return C.CDLL(so)


def test_plain_loop_equals_the_model(pkg, baseline):
    ox = pkg.orbx
    baseline.pnp_loop.argtypes = [C.POINTER(ox.PnpJob), C.c_int]
    keys = [sc.keys()[i] for i in (0, 1, 2, 3, 5, 12)]
    arr = (ox.PnpJob * len(keys))()
    keep = []
    for i, key in enumerate(keys):
        J, k, out = ox._pnp_job(sc.job(*key), "t")
        arr[i] = J
        keep.append((k, out))
    assert baseline.pnp_loop(arr, len(keys)) == 0
    for key, (k, out) in zip(keys, keep):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(out, sc.table(*key))), key
