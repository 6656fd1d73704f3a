"""orbx_debug_lba_profile and orbx_debug_eg_profile (LaunchProfile, csrc/orbx_resident.h): the slot counts, that a profiled call returns the
bytes of an unprofiled one, and that the launches counted per slot are the ones the report's iterations and trials imply.  The launch
counts are what pins the host Levenberg loop (lm_host_loop, csrc/orbx_lm.h): a launch or a linearisation more per trial shows here.

Scenes: the local bundle adjustment on 3-2-64-mixed, the global one on 1-60-stereo (the smallest scene of gba_scene.all_tags() that runs an
iteration; no_points and no_edges are smaller and would check 0 == 0), the essential graph on 5-free."""
import ctypes as C

import numpy as np
import pytest

import eg_scene as es
import gba_scene as gs
import lba_scene as ls

LBA_SLOTS = ("INIT", "ACTIVE", "LINEARIZE", "KF", "REDUCE", "PREP", "SCHUR", "SOLVE", "UPDATE", "ERRORS", "CLASSIFY", "FINISH")
EG_SLOTS = ("SETUP", "LINEARIZE", "ROWS", "REDUCE", "FILL", "SOLVE", "UPDATE", "ERRORS", "FINISH", "POINTS")


def same_bytes(a, b):
    return a.keys() == b.keys() and all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)


def profiled(entry, slots, call):
    """call() unprofiled, then profiled -> (the profiled result, {slot: launches}); asserts what does not depend on the solver"""
    plain = call()
    assert entry(1, None, None) == 0
    got = call()
    ms, cnt = np.full(len(slots) + 2, -1.0), np.full(len(slots) + 2, -1, np.int32)
    assert entry(0, ms.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p)) == len(slots)
    assert (ms[len(slots):] == -1.0).all() and (cnt[len(slots):] == -1).all()           # nothing behind the slots is written
    assert same_bytes(got, plain), "the profiled call returns other bytes"
    assert (cnt[:len(slots)] >= 0).all() and (ms[:len(slots)] >= 0.0).all() and (ms[:len(slots)][cnt[:len(slots)] == 0] == 0.0).all()
    assert same_bytes(call(), plain)                                                    # the read-out switched the profile off:
    again = np.zeros(len(slots), np.int32)                                              # a further call adds nothing
    assert entry(0, None, again.ctypes.data_as(C.c_void_p)) == len(slots)
    assert again.tobytes() == cnt[:len(slots)].tobytes()
    return got, dict(zip(slots, (int(v) for v in cnt)))


def check_ba_counts(n, iterations, trials, active_kf, rounds):
    I, T = sum(iterations), sum(trials)
    with_rows = [k for k in range(len(trials)) if active_kf[k] > 0]
    assert I > 0 and T >= I
    assert n["LINEARIZE"] == I and n["REDUCE"] == I + T
    assert n["PREP"] == T and n["UPDATE"] == T and n["ERRORS"] == T
    assert n["INIT"] == 1 and n["FINISH"] == 1 and n["ACTIVE"] == rounds
    assert n["KF"] == sum(iterations[k] for k in with_rows)
    assert n["SCHUR"] == sum(trials[k] for k in with_rows) and n["SOLVE"] == n["SCHUR"]
    assert len(with_rows) == len(trials) and n["SCHUR"] == T                           # the scenes are chosen so: every round has rows


@pytest.mark.gpu
def test_local_bundle_adjustment(pkg):
    pr = dict(ls.all_scenes())["3-2-64-mixed"]["problem"]
    got, n = profiled(pkg.lib().orbx_debug_lba_profile, LBA_SLOTS, lambda: pkg.local_bundle_adjustment(pr))
    print(got["iterations"], got["trials"], got["n_active_kf"], n)
    assert got["stopped"] == 0
    check_ba_counts(n, list(got["iterations"]), list(got["trials"]), list(got["n_active_kf"]), rounds=2)
    assert n["CLASSIFY"] == 2


@pytest.mark.gpu
def test_bundle_adjustment(pkg):
    sc, opts = gs.case("1-60-stereo")
    got, n = profiled(pkg.lib().orbx_debug_lba_profile, LBA_SLOTS, lambda: pkg.bundle_adjustment(sc["problem"], **opts))
    print(got["iterations"], got["trials"], got["n_active_kf"], n)
    assert got["stopped"] == 0
    check_ba_counts(n, [got["iterations"]], [got["trials"]], [got["n_active_kf"]], rounds=1)
    assert n["CLASSIFY"] == 0


@pytest.mark.gpu
def test_essential_graph(pkg):
    pr, opts = es.case("5-free")
    got, n = profiled(pkg.lib().orbx_debug_eg_profile, EG_SLOTS, lambda: pkg.optimize_essential_graph(pr, **opts))
    print(got["iterations"], got["trials"], n)
    I, T = got["iterations"], got["trials"]
    assert I > 0 and T >= I
    assert n["LINEARIZE"] == I and n["ROWS"] == I
    assert n["FILL"] == T and n["SOLVE"] == T and n["UPDATE"] == T and n["ERRORS"] == T
    assert n["REDUCE"] == I + T
    assert n["SETUP"] == 1 and n["FINISH"] == 1
    assert n["POINTS"] == (1 if len(pr["Xw"]) else 0)
