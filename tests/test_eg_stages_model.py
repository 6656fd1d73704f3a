"""tests/eg_model.py's stages() and the inputs of tests/test_eg_stages.py on the CPU: the honest model passes every check the GPU test
puts to the device (tests/eg_stage_checks.py), every deliberate error of the model fails the check named for it or moves the rows it can
touch by 16 x their bound, the designed tables reach the paths they were designed for, and the measured spreads are the ones the GPU
test's docstring quotes (python tools/eg_spread.py --stages)."""
import numpy as np
import pytest

import eg_model as em
import eg_scene as es
import eg_stage_checks as ck

# python tools/eg_spread.py --stages: case -> (rows, floor, largest spread, rows whose bound exceeds 1e-10), rounded up in the fourth digit
MEASURED = {"log-free": (142, 5.275e-16, 2.915e-14, ()), "log-fix": (282, 3.954e-16, 1.041e-06, (107, 109, 115, 117)),
            "exp-free": (33, 4.165e-16, 1.111e-12, ()), "exp-fix": (33, 2.030e-16, 1.111e-12, ()), "long-free": (300, 1.777e-14, 1.280e-13, ())}
# the smallest change / bound of the mutations seen under the bound, rounded down
MARGINS = {("b_minus_one", "log-free"): 1.70e+03, ("b_minus_one", "log-fix"): 3.77e+03, ("lu_wrong_row", "log-free"): 6.0e+12,
           ("lu_wrong_row", "log-fix"): 3.0e+12}


def quantity(name):
    return "trial" if name.startswith("exp-") else "err"


@pytest.mark.parametrize("name", es.STAGE_CASES)
def test_the_model_passes_every_check(name):
    c, m = es.stage_case(name), es.stage_models(name)[0]
    pr, lam = c["problem"], c["lam"]
    for check in ("setup", "probe", "record", "rows", "scatter", "update"):
        assert ck.run_check(check, pr, m, lam, m) == [], check
    assert ck.check_status(pr, m) == []
    if c["x"] is None:
        assert m["solve_ok"] == 1


@pytest.mark.parametrize("name", es.STAGE_CASES)
def test_spreads_are_the_measured_ones(name):
    c, runs = es.stage_case(name), es.stage_models(name)
    bound, spread, floor = ck.row_bounds([r[quantity(name)] for r in runs])
    big = tuple(int(i) for i in np.nonzero(bound > 1e-10)[0])
    print(name, len(bound), floor, spread.max(), big)
    assert len(big) <= 0.02 * len(bound)
    if name in MEASURED:
        rows, fl, mx, named = MEASURED[name]
        assert len(bound) == rows and floor <= fl and spread.max() <= mx and big == named
        assert floor >= 0.99 * fl and spread.max() >= 0.99 * mx                  # the docstrings quote what is measured, not a ceiling
    else:
        assert spread.max() <= 7.106e-15 and not big                             # the shapes: fixed_in_middle, fixed_at_both_ends


def test_the_log_table_reaches_every_path():
    """by evaluation 0 of its rows alone: the four branches of Sim3::log, the three pivot rows and the second exchange taken and not"""
    for name in ("log-free", "log-fix"):
        m = es.stage_models(name)[0]
        branch, (piv, second) = m["paths"]["log_rows"][0], m["paths"]["rows"][0]
        E = len(es.stage_case(name)["labels"])
        assert len(branch) == len(piv) == len(second) == E
        print(name, np.bincount(branch, minlength=4), np.bincount(piv, minlength=3), np.bincount(second.astype(int), minlength=2))
        assert (np.bincount(branch, minlength=4) > 0).all()
        assert (np.bincount(piv, minlength=3) > 0).all() and second.any() and (~second).any()
    rows = dict(es.log_rows(1))
    assert len(rows) == 7 * 5 * 8 + 2 and len(es.log_rows(0)) == 7 * 5 * 4 + 2
    q = rows["norm 1 + 1e-3"][:4]
    assert abs(np.linalg.norm(q) - (1.0 + 1e-3)) < 1e-15 and abs(np.linalg.norm(rows["-q"][:4]) - 1.0) < 1e-15 and rows["-q"][3] < 0
    pr, _ = es.log_table(0)
    m = es.stage_models("log-free")[0]
    assert (m["meas"] == es.IDENTITY).all()                                      # every measurement is the identity, exactly
    assert ck.same(m["err"][:, 0], em.log(pr["S_corrected"], em.Libm()))         # so the start error of row r is log(D_r)


def test_the_exp_table_reaches_every_path():
    for name, scale_branches in (("exp-free", 4), ("exp-fix", 2)):
        c = es.stage_case(name)
        g = em.Graph(c["problem"], em.Libm())
        paths = em.new_paths()
        x = np.array(c["x"])
        if c["problem"]["fix_scale"]:
            x[6::7] = 0.0
        for r in range(g.F):
            em.exp_paths(x[7 * r:7 * r + 7], paths)
        print(name, paths["exp"], paths["quat"])
        assert sum(v > 0 for v in paths["exp"]) == scale_branches and all(paths["quat"])
    vs = em.new_paths()
    em.vscw(es.stage_case("exp-free")["problem"], vs)
    assert all(vs["quat"]), vs["quat"]                                            # the keyframe rotations: all four branches of Quaternion(Matrix3)


def test_shapes_are_their_case():
    for E in (1, 7, 8, 9, 17):
        assert len(es.shape(f"edges-{E}")["edge_i"]) == E
    fixed_ends = {}
    for tag in es.SHAPES:
        pr = es.shape(tag)
        k0 = int(np.nonzero(pr["fixed"])[0][0])
        assert pr["fixed"].sum() == 1
        fixed_ends[tag] = (k0 in pr["edge_i"], k0 in pr["edge_j"])
    assert fixed_ends["edges-9"] == (False, True) and fixed_ends["fixed-is-i"] == (True, False) and fixed_ends["fixed-has-no-edge"] == (False, False)
    assert fixed_ends["fixed_at_both_ends"] == (True, True)
    assert {s["fix_scale"] for s in map(es.shape, es.SHAPES)} == {0, 1}
    pr = es.long_chain()
    assert len(pr["fixed"]) - 1 == 260 and len(pr["edge_i"]) == 300
    pr = es.shape("edges-9")                                                      # what the mutations' cases need
    row = ck.lists(pr)[0]
    assert ((pr["edge_kind"] != 0) & ((pr["noncorrected"][pr["edge_i"]] >= 0) | (pr["noncorrected"][pr["edge_j"]] >= 0))).any()
    assert ((row[pr["edge_i"]] >= 0) & (row[pr["edge_j"]] >= 0) & (row[pr["edge_i"]] < row[pr["edge_j"]])).any()


@pytest.mark.parametrize("mut", sorted(ck.SEEN_BY))
def test_every_mutation_is_seen(mut):
    """test 8 on the model: a mutation seen by an equal-bytes check makes that check fail; one seen under the bound moves every row it can
    touch by at least 16 x the row's bound.  None is left "not told from the truth"."""
    check, kind = ck.SEEN_BY[mut]
    for name in ck.MUTATION_CASES[mut]:
        c, runs, bad = es.stage_case(name), es.stage_models(name), es.stage_models(name, mut)[0]
        if kind == "bytes":
            found = ck.run_check(check, c["problem"], bad, c["lam"], runs[0])
            print(mut, name, found[:1])
            assert found
        else:
            rows, ratio, change, bound = ck.margin(mut, runs, bad)
            print(mut, name, len(rows), ratio, change, bound)
            assert len(rows) >= 8 and ratio >= 16 and ratio >= MARGINS[(mut, name)]


def test_the_mutation_lists_are_whole():
    assert set(em.STAGE_MUTATIONS) <= set(ck.SEEN_BY) and set(ck.SEEN_BY) == set(ck.MUTATION_CASES)
    # of the six older ones, t_not_divided is held by Tcw == float32(recover(S)) and lambda_diag by the host-loop test (tests/test_eg_stages.py)
    assert set(em.MUTATIONS) - set(ck.SEEN_BY) == {"t_not_divided", "lambda_diag"}


def test_one_iteration_leaves_lambda_from_1e_16():
    """the model's side of test_eg_stages.py's host-loop test: with iterations = 1 every scene runs exactly one trial, accepts it and ends
    with lambda in [1e-16 / 3, 2e-16 / 3]; from tau x the largest diagonal entry (the mutation "lambda_diag") it ends above 1e-5"""
    for tag in es.all_tags(big=False):
        pr, opts = es.case(tag)
        if opts["iterations"] == 0 or len(pr["edge_i"]) == 0:
            continue
        a, b = em.optimize(pr, iterations=1), em.optimize(pr, iterations=1, mutation="lambda_diag")
        assert a["trials"] == 1 and 1e-16 * (1.0 / 3.0) <= a["lambda"] <= 1e-16 * (2.0 / 3.0), tag
        assert b["lambda"] > 1e-5, tag


def test_the_python_mirror_is_the_header(pkg):
    """orbx_eg_stages' fields in include/orbx.h, in order, are EgStages' (every one a pointer); the call is declared, exported and typed"""
    import ctypes as C
    import os
    import re
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "orbx.h")).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\} orbx_eg_stages;", src).group(1)
    names = re.findall(r"\*\s*([A-Za-z_]+)", body)
    assert names == [f[0] for f in pkg.orbx.EgStages._fields_] and C.sizeof(pkg.orbx.EgStages) == len(names) * C.sizeof(C.c_void_p)
    assert set(pkg.orbx.EG_STAGES) | {"n_pairs"} == set(names)
    m = re.search(r"\bint\s+orbx_debug_eg_stages\s*\(([^)]*)\)\s*;", src)
    assert m and len(m.group(1).split(",")) == 6 and len(pkg.lib().orbx_debug_eg_stages.argtypes) == 6
    assert (int(re.search(r"#define ORBX_EG_STAGES_MAX_N (\d+)", src).group(1)), int(re.search(r"#define ORBX_EG_STAGES_MAX_PROBED (\d+)", src).group(1))) == \
        (pkg.orbx.EG_STAGES_MAX_N, pkg.orbx.EG_STAGES_MAX_PROBED)
