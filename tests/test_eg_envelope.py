"""orbx_optimize_essential_graph2: the essential graph with the system stored and factored as an envelope (orbx_ldlt_env.hip), and the
structure query orbx_eg_envelope.

The envelope solver performs the dense solver's operations in the dense solver's order minus terms that are an exact zero, so ENVELOPE
gives every output and every report field of DENSE with numpy.array_equal, no tolerance (whether the bytes were equal too is printed: a
-0 in place of a +0 is the one way they can differ); DENSE through the new entry point gives the BYTES of the old entry point.  Past the
dense solver's 1536 free keyframes there is nothing to compare with but the model's evaluation of chi2 at the returned estimates, under
BOUND_CHI2 of tests/test_essential_graph.py, and what that file asserts of every call.

The adaptor test: -DORBX_EG_ORDER_BY_ID makes adapter/essential/OptimizeEssentialGraph.cc index the keyframes by mnId; a scene file that
lists them shuffled then leaves the map as the scene in mnId order does without the define.  (The LoopConnections edges follow the pointer
order of the std::map that holds them, with or without the define; the shuffle keeps the two keyframes that have one in their order.)"""
import os
import subprocess

import numpy as np
import pytest

import eg_model as em
import eg_scene as es
import pose_model as pm
import test_eg_adapter as tea
from test_essential_graph import BOUND_CHI2
from tools.pose_spread import chi2_diff

f32 = np.float32
DENSE, ENVELOPE, AUTO = 0, 1, 2
W = 32
_cache = {}


def count(pr):
    """the envelope rule of include/orbx.h, restated -> (entries, triangle)"""
    fixed = np.asarray(pr["fixed"]) != 0
    F = int((~fixed).sum())
    row = np.full(len(fixed), -1)
    row[~fixed] = np.arange(F)
    lowest = np.arange(F)
    for ri, rj in zip(row[pr["edge_i"]], row[pr["edge_j"]]):
        if ri >= 0 and rj >= 0:
            lowest[max(ri, rj)] = min(lowest[max(ri, rj)], ri, rj)
    first = np.repeat(7 * lowest // W * W, 7)
    n = 7 * F
    return int((np.arange(n) - first + 1).sum()), n * (n + 1) // 2


def shuffled(pr, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return es.permute(pr, rng.permutation(len(pr["fixed"])))


def big(F, fix):
    if (F, fix) not in _cache:
        _cache[(F, fix)] = es.make(F, fix, 9400 + F + fix)
    return _cache[(F, fix)]


def equal(a, b):
    return a.keys() == b.keys() and all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in a)


def same_bytes(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)


def test_structure_query(pkg):
    """host only: the library loads and answers without a device"""
    assert pkg.orbx.ldlt_panel_width() == W
    for F in (9, 37, 150):
        pr = es.make(F, 0, 1)
        got = pkg.orbx.eg_envelope(pr)
        assert got == count(pr), F
        more = pkg.orbx.eg_envelope(shuffled(pr, 40 + F))
        assert more == count(shuffled(pr, 40 + F)) and more[1] == got[1] and (more[0] > got[0] or F == 9), F
    assert pkg.orbx.eg_envelope(es.make(150, 0, 1)) == (54943, 551775)
    one = es.make(0, 0, 1)                                                     # the fixed keyframe alone
    assert pkg.orbx.eg_envelope(one) == (0, 0)
    bad = dict(es.make(9, 0, 1)); bad["fixed"] = np.zeros(10, np.uint8)
    with pytest.raises(pkg.OrbxError):
        pkg.orbx.eg_envelope(bad)


def test_an_envelope_beyond_the_limit_is_refused_before_any_device_work(pkg):
    L = pkg.lib()
    sh = shuffled(big(4095, 1), 77)
    entries, triangle = pkg.orbx.eg_envelope(sh)
    assert entries > pkg.orbx.EG_MAX_ENVELOPE == 1 << 27 and entries <= triangle == 28665 * 28666 // 2
    before = L.orbx_debug_thread_contexts()
    for solver in (ENVELOPE, AUTO):
        with pytest.raises(pkg.OrbxError) as e:
            pkg.optimize_essential_graph(sh, solver=solver)
        assert e.value.code == -2 and str(entries) in str(e.value) and str(1 << 27) in str(e.value)
    with pytest.raises(pkg.OrbxError) as e:
        pkg.optimize_essential_graph(sh, solver=DENSE)
    assert e.value.code == -2 and "1536" in str(e.value)
    with pytest.raises(pkg.OrbxError) as e:
        pkg.optimize_essential_graph(es.make(5, 0, 1), solver=3)
    assert e.value.code == -1 and "solver" in str(e.value)
    assert L.orbx_debug_thread_contexts() == before


TAGS = ["37-free", "37-fix", "150-free", "vertex_without_edge", "fixed_in_middle", "two_edges_one_pair", "no_edges", "no_iterations", "37-free-shuffled"]


@pytest.mark.gpu
@pytest.mark.parametrize("tag", TAGS)
def test_envelope_equals_dense(pkg, tag):
    if tag == "37-free-shuffled":
        pr, opts = es.case("37-free")
        pr = shuffled(pr, 41)
    else:
        pr, opts = es.case(tag)
    old = pkg.optimize_essential_graph(pr, **opts)
    dense = pkg.optimize_essential_graph(pr, solver=DENSE, **opts)
    env = pkg.optimize_essential_graph(pr, solver=ENVELOPE, **opts)
    auto = pkg.optimize_essential_graph(pr, solver=AUTO, **opts)
    entries, triangle = pkg.orbx.eg_envelope(pr)
    print(f"{tag}: envelope {entries} of {triangle}, iterations {env['iterations']} trials {env['trials']} failed solves {env['n_solve_failed']} "
          f"chi2 {env['chi2_start']:.6g} -> {env['chi2']:.6g}; envelope bytes equal to dense: {same_bytes(env, dense)}")
    assert same_bytes(dense, old)
    assert equal(env, dense), [k for k in dense if not np.array_equal(np.asarray(env[k]), np.asarray(dense[k]))]
    assert equal(auto, dense) and equal(auto, env)
    if len(pr["edge_i"]) and opts["iterations"]:
        assert env["iterations"] > 0 and env["n_solve_failed"] == 0


@pytest.mark.gpu
def test_at_the_limit_of_the_dense_solver(pkg):
    pr = big(1536, 0)
    dense = pkg.optimize_essential_graph(pr, solver=DENSE)
    env = pkg.optimize_essential_graph(pr, solver=ENVELOPE)
    print(f"1536 free: iterations {env['iterations']} trials {env['trials']}; envelope bytes equal to dense: {same_bytes(env, dense)}")
    assert env["trials"] > 0 and equal(env, dense)


def model_chi2(pr, S):
    g = em.Graph(pr, em.Libm(None))
    return float(pm.ordered_sum(em.chi2_of(em.errors(g, S)), "asc"))


@pytest.mark.gpu
@pytest.mark.parametrize("F", [1537, 4095])
def test_past_the_limit_of_the_dense_solver(pkg, F):
    pr = big(F, 1)
    with pytest.raises(pkg.OrbxError) as e:
        pkg.optimize_essential_graph(pr)
    assert e.value.code == -2
    got = pkg.optimize_essential_graph(pr, solver=ENVELOPE)
    exp = model_chi2(pr, got["S"])
    print(f"{F} free: envelope {pkg.orbx.eg_envelope(pr)}, iterations {got['iterations']} trials {got['trials']} chi2 {got['chi2_start']:.6g} -> "
          f"{got['chi2']:.6g}, the model at the returned S {exp:.6g}: {chi2_diff(exp, got['chi2']):.3e} (bound {BOUND_CHI2:.3e})")
    assert got["n_free"] == F and got["n_solve_failed"] == 0 and got["iterations"] > 0 and got["chi2"] < got["chi2_start"]
    assert got["Tcw"][:, :3].tobytes() == em.recover(got["S"]).astype(f32).tobytes()
    assert (got["Tcw"][:, 3] == np.array([0, 0, 0, 1], f32)).all()
    assert got["Xw"].tobytes() == got["point"].astype(f32).tobytes()
    assert chi2_diff(exp, got["chi2"]) <= BOUND_CHI2
    assert same_bytes(got, pkg.optimize_essential_graph(pr, solver=AUTO))      # a second call, and AUTO takes the envelope here


def reorder(kfs, connections, pts, order):
    """the stub map with its keyframes listed in another order: order[new] = old; every index into the list follows"""
    new_of = {old: new for new, old in enumerate(order)}
    out = []
    for old in order:
        K = dict(kfs[old])
        K["parent"] = new_of[K["parent"]] if K["parent"] >= 0 else -1
        K["loop"] = [new_of[b] for b in K["loop"]]
        K["cov"] = [(new_of[b], w) for b, w in K["cov"]]
        out.append(K)
    con = {new_of[a]: [new_of[b] for b in lst] for a, lst in connections.items()}
    return out, con, [dict(P, ref=new_of[P["ref"]]) for P in pts], new_of


@pytest.mark.gpu
def test_adaptor_orders_the_keyframes_by_id(pkg, tmp_path, monkeypatch):
    kfs, connections, pts, fix = tea.stub_map()
    by_id = sorted(range(len(kfs)), key=lambda k: kfs[k]["id"])
    rng = np.random.Generator(np.random.PCG64(9950))
    mixed = [int(k) for k in rng.permutation(len(kfs))]
    with_con = sorted(connections)                                             # the keyframes that hold LoopConnections: kept in their order
    slots = sorted(mixed.index(k) for k in with_con)
    for slot, k in zip(slots, with_con):
        mixed[slot] = k
    assert mixed != by_id and mixed != list(range(len(kfs))) and sorted(mixed) == sorted(by_id) == list(range(len(kfs)))
    plain = tea.build_driver(str(tmp_path))
    ordered = os.path.join(str(tmp_path), "adapter_eg_driver_by_id")
    pkg_dir = os.path.join(tea.ROOT, "orb-slam2_amd")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-DORBX_EG_ORDER_BY_ID"] + tea.INC + tea.SOURCES +
                          ["-L", pkg_dir, "-lorbx", "-lpthread", "-Wl,-rpath," + pkg_dir, "-o", ordered])
    res = {}
    for name, exe, order in (("by_id", plain, by_id), ("mixed", ordered, mixed)):
        k2, c2, p2, new_of = reorder(kfs, connections, pts, order)
        monkeypatch.setattr(tea, "LOOP", new_of[tea.LOOP])
        monkeypatch.setattr(tea, "CUR", new_of[tea.CUR])
        path = str(tmp_path / (name + ".txt"))
        tea.write_scene(path, k2, c2, p2, fix)
        kf, pt = tea.run_driver(exe, path)
        monkeypatch.undo()
        res[name] = ({k2[k]["id"]: kf[k] for k in range(len(k2))}, pt)
    (kf_a, pt_a), (kf_b, pt_b) = res["by_id"], res["mixed"]
    assert kf_a.keys() == kf_b.keys() and pt_a.keys() == pt_b.keys()
    for i in kf_a:
        assert kf_a[i]["setpose"] == kf_b[i]["setpose"] and kf_a[i]["Tcw"].tobytes() == kf_b[i]["Tcw"].tobytes(), i
    for j in pt_a:
        assert pt_a[j]["set"] == pt_b[j]["set"] and pt_a[j]["pos"].tobytes() == pt_b[j]["pos"].tobytes(), j
    moved = [i for i in kf_a if kf_a[i]["setpose"] and not np.array_equal(kf_a[i]["Tcw"], np.asarray(kfs[[K["id"] for K in kfs].index(i)]["Tcw"], f32))]
    assert moved                                                               # the call did something
