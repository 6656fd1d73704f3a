"""tests/eg_model.py and tests/eg_scene.py on the CPU: every scene of the OptimizeEssentialGraph GPU tests stays within the measured spread
across the model's variants, the scenes between them visit all four branches of Sim3::log, the deliberate errors move what they should,
a noise-free graph is solved to rounding, and the exact cases are exact.  The constants are tests/test_essential_graph.py's:

    python tools/eg_spread.py
    SPREAD_S = 1.476e-04  SPREAD_POINT = 1.919e-04  SPREAD_CHI2 = 9.938e-06  (x 64: 9.446e-03, 1.228e-02, 6.360e-04)"""
import numpy as np
import pytest

import eg_model as em
import eg_scene as es
from tools.eg_spread import out_diff, s_diff, touches
from tools.lba_spread import points_diff
from tools.pose_spread import chi2_diff

f32 = np.float32
SPREAD_S = 1.476e-04
SPREAD_POINT = 1.919e-04
SPREAD_CHI2 = 9.938e-06

_cache = {}


def runs(tag):
    if tag not in _cache:
        pr, opts = es.case(tag)
        _cache[tag] = (pr, opts, es.variants(pr, opts))
    return _cache[tag]


@pytest.mark.parametrize("tag", es.all_tags())
def test_scene_within_the_spread(tag):
    pr, opts, rs = runs(tag)
    a = rs[0]
    assert a["n_free"] == len(pr["fixed"]) - 1
    for r in rs[1:]:
        assert s_diff(a["S"], r["S"]) <= SPREAD_S and points_diff(a["point"], r["point"]) <= SPREAD_POINT
        assert chi2_diff(a["chi2"], r["chi2"]) <= SPREAD_CHI2
    if len(pr["edge_i"]) and opts["iterations"]:
        assert all(r["chi2"] < r["chi2_start"] for r in rs)


def test_all_four_log_branches_are_visited():
    total = [0, 0, 0, 0]
    for tag in es.all_tags():
        total = [p + q for p, q in zip(total, runs(tag)[2][0]["branches"])]
    assert all(total), total
    assert runs("half_radian")[2][0]["decisions"] and em.optimize(runs("half_radian")[0], iterations=1)["branches"][3] > 0   # acos at the start


def test_scenes_are_their_case():
    pr = es.case("two_edges_one_pair")[0]
    pairs = [(min(i, j), max(i, j)) for i, j in zip(pr["edge_i"], pr["edge_j"])]
    assert pairs.count((5, 6)) == 3
    pr = es.case("vertex_without_edge")[0]
    assert 4 not in pr["edge_i"] and 4 not in pr["edge_j"] and not pr["fixed"][4]
    pr = es.case("fixed_in_middle")[0]
    assert pr["fixed"][4] and pr["fixed"].sum() == 1
    pr = es.case("fixed_at_both_ends")[0]
    k0 = int(np.nonzero(pr["fixed"])[0][0])
    assert k0 in pr["edge_i"] and k0 in pr["edge_j"]
    for F in es.SIZES:
        for fix in (0, 1):
            pr = es.case(es.tag_of(F, fix))[0]
            assert len(pr["fixed"]) == F + 1 and pr["fix_scale"] == fix and (pr["edge_kind"] == 0).any() and (pr["edge_kind"] == 1).any()
            if not fix:
                assert not 0.95 < pr["S_corrected"][-1, 7] < 1.05          # a scale correction of 10 - 30 %


@pytest.mark.parametrize("m", em.MUTATIONS)
def test_mutation_moves_the_result(m):
    """each deliberate error changes the output of at least one scene it can touch by more than the spread (which scenes, and by how
    much against the GPU bound: tools/eg_spread.py --mutations, tests/test_essential_graph.py)"""
    tags = {"lambda_diag": "10-free", "x6_not_zeroed": "10-fix", "normal_from_vscw": "10-free", "normalise": "5-fix", "t_not_divided": "10-free",
            "bta_untransposed": "two_edges_one_pair"}
    pr, opts = es.case(tags[m])
    assert touches(m, pr, opts)
    base, mut = runs(tags[m])[2][0], em.optimize(pr, mutation=m, **opts)
    d = out_diff(base, mut)
    print(m, tags[m], d)
    if m == "normalise":       # the quaternions are unit ones to rounding: normalising them moves the result, but inside the spread
        assert 0.0 < d <= SPREAD_S
    else:
        assert d > max(SPREAD_S, SPREAD_POINT, SPREAD_CHI2)


@pytest.mark.parametrize("tag", ["consistent-free", "consistent-fix"])
def test_noise_free_graph_is_solved(tag):
    pr, opts, rs = runs(tag)
    truth = es.consistent_truth(pr)
    for r in rs:
        assert r["chi2"] < 1e-12 * r["chi2_start"]
        assert s_diff(truth, r["S"]) <= SPREAD_S


def test_free_scale_stalls_in_the_branch_without_its_minus_one():
    """reported, not hidden: the same noise-free graph with a start that is off in rotation and scale too enters the branch of Sim3::log
    whose B lacks the -1 (eg_scene.make) and ends at chi2 = 8.6e-05 x the start after ten rejected trials"""
    pr, opts, rs = runs("stall-free")
    a = rs[0]
    print(a["chi2"] / a["chi2_start"], a["branches"])
    assert a["branches"][2] > 0 and a["trials"] - a["iterations"] >= 9 and a["chi2"] > 1e-12 * a["chi2_start"]


def test_exact_cases():
    pr, opts, rs = runs("no_iterations")
    V = em.vscw(pr)
    for r in rs:                                   # the start through the recovery, exactly
        assert r["S"].tobytes() == V.tobytes() and r["pose"].tobytes() == em.recover(V).tobytes()
        assert r["point"].tobytes() == em.correct_points(pr, V, V).tobytes() and (r["iterations"], r["trials"]) == (0, 0)
    for tag in es.all_tags():
        pr, opts, rs = runs(tag)
        V = em.vscw(pr)
        k0 = int(np.nonzero(pr["fixed"])[0][0])
        has = np.zeros(len(pr["fixed"]), bool)
        has[pr["edge_i"]] = True; has[pr["edge_j"]] = True
        for r in rs:
            assert r["S"][k0].tobytes() == V[k0].tobytes()                   # the fixed keyframe's S_out is its vScw
            assert r["S"][~has].tobytes() == V[~has].tobytes()               # exp(0) * S is exact
            if pr["fix_scale"]:
                assert r["S"][:, 7].tobytes() == V[:, 7].tobytes()
    assert (~np.isin(np.arange(9), np.concatenate([es.case("vertex_without_edge")[0][k] for k in ("edge_i", "edge_j")]))).sum() == 1
