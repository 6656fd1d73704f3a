"""orbx_debug_eg_stages: every device stage of orbx_optimize_essential_graph held on its own -- one linearisation and one trial, what each
kernel left in device memory (include/orbx.h) -- on the small designed inputs of tests/eg_scene.py (STAGE_CASES).  The end-to-end
comparison of tests/test_essential_graph.py has a bound of 1e-2, because the function it tests is chaotic; nothing here runs a second
iteration, so nothing here inherits that.  The checks are tests/eg_stage_checks.py's, which tests/test_eg_stages_model.py puts to the model
and to every deliberate error of the model.

EQUAL BYTES, no tolerance (-ffp-contract=off: + - x / and sqrt in a stated order):
  setup    vS and meas are the model's.
  probe    eg_chi2(err[:, 0]) == echi: the probe kernel's evaluation 0 is the error the linearisation kernel squared.
  record   rec is the record numpy forms from the DEVICE's own err; rec[119] == echi; the blocks of a fixed end and, under fix_scale, rows
           and columns 6 and 13 are zeros.
  rows     Hd, bv, Off and the pair list are the ordered sums of the DEVICE's own rec in edge order.
  scatter  S's lower triangle is the scatter of the device's own Hd and Off with lambda on the diagonal and nowhere else, zeros outside the
           blocks; y == bv.
  update   sc is the seven-term sum of the device's own x and bv; the fixed keyframe keeps its estimate; under fix_scale x[6::7] == 0 and the
           trial's scale bits are the start's.
  status   status[2] is the largest |diagonal entry|.
  solve    x is tests/lba_model.py's ldlt_solve of the device's own S and y, as tests/test_ldlt_panel.py asks of the panel solver.

UNDER A BOUND
  status   status[0], status[1] against math.fsum of the device's own echi, sc within 256 eps x the sum of the magnitudes.
  solve    |S x - y| in longdouble <= 1e-9 n max |y|, tests/test_ldlt_panel.py's bound for a solution.
  err, trial  against the model per row: row_diff <= 64 x the row's own spread across the model's nudges None, 1, 2, floored at the table's
           median row spread (eg_stage_checks.row_bounds).  Measured on the model alone:

    python tools/eg_spread.py --stages
    STAGE log-free  err   rows 142 floor 5.274e-16 largest spread 2.914e-14 largest bound 1.865e-12 rows over 1e-10: 0
    STAGE log-fix   err   rows 282 floor 3.953e-16 largest spread 1.040e-06 largest bound 6.659e-05 rows over 1e-10: 4 (1.4 %)
        ROW 107 (theta 0.00447113968 axis (1, 1, 0) sigma 1.0001e-05)  spread 1.240e-07 bound 7.934e-06
        ROW 109 (theta 0.00447113968 axis (1, 1, 0) sigma -1.0001e-05) spread 4.530e-07 bound 2.899e-05
        ROW 115 (theta 0.00447113968 axis (1, 2, 3) sigma 1.0001e-05)  spread 7.147e-07 bound 4.574e-05
        ROW 117 (theta 0.00447113968 axis (1, 2, 3) sigma -1.0001e-05) spread 1.040e-06 bound 6.659e-05
    STAGE exp-free  trial rows 33 floor 4.164e-16 largest spread 1.110e-12 largest bound 7.105e-11
    STAGE exp-fix   trial rows 33 floor 2.029e-16 largest spread 1.110e-12 largest bound 7.105e-11
    STAGE long-free err   rows 300 floor 1.776e-14 largest spread 1.279e-13 largest bound 8.185e-12
    STAGE shape-*   err   largest bound 4.547e-13 (fixed_in_middle, fixed_at_both_ends)

  The four rows over 1e-10 are one corner: the largest rotation that still counts as small (1e-6 rad under acos(1 - eps)) about an axis
  that is no coordinate axis, with |sigma| just over eps -- the branch of Sim3::log whose B lacks its -1 (tests/eg_scene.py: make), at the
  point where that B = 1e15 multiplies the largest Omega^2 the branch admits (2e-5): W's entries are 2e10 and cancel against each other.
  A mutation seen under the bound moves every row it can touch by at least 16 x that row's bound (MARGINS below, asserted here and, on
  the model, in tests/test_eg_stages_model.py):

    MUTATION b_minus_one   log-free 20 rows, smallest change / bound 1.702e+03; log-fix 40 rows, 3.776e+03
    MUTATION lu_wrong_row  log-free  8 rows, smallest change / bound 6.030e+12; log-fix 16 rows, 3.036e+12

THE HOST LOOP: test_one_iteration_leaves_lambda_from_1e_16 holds setUserLambdaInit(1e-16) (the mutation "lambda_diag").
Each test prints its figures before it asserts."""
import ctypes as C
import math

import numpy as np
import pytest

import eg_scene as es
import eg_stage_checks as ck
import lba_model

f32 = np.float32
_dumps = {}


def dump(pkg, name):
    """the device's stages of a case, fetched once"""
    if name not in _dumps:
        c = es.stage_case(name)
        want = [k for k in pkg.orbx.EG_STAGES if k != "S" or c["S"]]
        _dumps[name] = pkg.orbx.eg_stages(c["problem"], c["lam"], x=c["x"], trial=True, want=want)
    return _dumps[name]


def check(found):
    for f in found:
        print("FOUND:", f)
    assert not found


@pytest.mark.gpu
@pytest.mark.parametrize("name", es.STAGE_CASES)
def test_equal_bytes(pkg, name):
    """tests 1 - 4 of the list above (setup, probe, record, rows, scatter, update, status[2]) and the sums of status"""
    c, d, model = es.stage_case(name), dump(pkg, name), es.stage_models(name)[0]
    pr, lam = c["problem"], c["lam"]
    assert d["n_pairs"] == model["n_pairs"] and d["err"].shape == model["err"].shape
    check(ck.check_setup(pr, d, model))
    check(ck.check_probe(pr, d))
    check(ck.check_record(pr, d))
    check(ck.check_rows(pr, d))
    if c["S"]:
        check(ck.check_scatter(pr, d, lam))
    else:
        assert ck.same(d["y"], d["bv"].reshape(-1))
    check(ck.check_update(pr, d, lam))
    check(ck.check_status(pr, d))
    if c["x"] is not None:
        x = np.array(c["x"])
        if pr["fix_scale"]:
            x[6::7] = 0.0
        assert ck.same(d["x"], x) and d["solve_ok"] == -1           # the update read x_in, and zeroed its scale entries under fix_scale
    assert d["status_lin"][1] == 0.0 and d["status_lin"][3] == 0.0 and ck.same(d["status_trial"][2], d["status_lin"][2])


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in es.STAGE_CASES if not n.startswith("exp-")])
def test_errors_match_the_model(pkg, name):
    """test 5: all 29 evaluations of every edge"""
    c, d, runs = es.stage_case(name), dump(pkg, name), es.stage_models(name)
    bound, spread, floor = ck.row_bounds([r["err"] for r in runs])
    diff = ck.row_diff(runs[0]["err"], d["err"])
    worst = int(np.argmax(diff - bound))
    print(f"{name}: rows {len(diff)} floor {floor:.3e} largest difference {diff.max():.3e} largest bound {bound.max():.3e}; row {worst} "
          f"({c['labels'][worst]}) difference {diff[worst]:.3e} bound {bound[worst]:.3e}")
    for i in np.nonzero(bound > 1e-10)[0]:
        print(f"  row {i} ({c['labels'][i]}) difference {diff[i]:.3e} bound {bound[i]:.3e}")
    assert (bound > 1e-10).sum() <= 0.02 * len(bound)
    assert (diff <= bound).all(), [(int(i), c["labels"][i], float(diff[i]), float(bound[i])) for i in np.nonzero(~(diff <= bound))[0]]
    if name.startswith("log-"):                                                  # no rotation, scale 1: log(1) = 0 is the one library call, W = I
        plain = [i for i, l in enumerate(c["labels"]) if l.startswith("theta 0 ") and l.endswith("sigma 0")]
        assert len(plain) == 5 and ck.same(d["err"][plain, 0], runs[0]["err"][plain, 0])
    if name.startswith("log-"):                                                  # test 8: what is seen under this bound is seen with a margin of 16
        for mut in ("b_minus_one", "lu_wrong_row"):
            rows, ratio, change, big = ck.margin(mut, runs, es.stage_models(name, mut)[0])
            print(f"  {mut}: {len(rows)} rows, smallest change {change:.3e}, smallest change / bound {ratio:.3e}")
            assert len(rows) and ratio >= 16


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["exp-free", "exp-fix"])
def test_trial_estimates_match_the_model(pkg, name):
    """test 5: Sim3(x) * S for the designed x of the exp table"""
    c, d, runs = es.stage_case(name), dump(pkg, name), es.stage_models(name)
    bound, spread, floor = ck.row_bounds([r["trial"] for r in runs])
    diff = ck.row_diff(runs[0]["trial"], d["trial"])
    worst = int(np.argmax(diff - bound))
    print(f"{name}: rows {len(diff)} floor {floor:.3e} largest difference {diff.max():.3e} largest bound {bound.max():.3e}; row {worst} "
          f"({c['labels'][worst]}) difference {diff[worst]:.3e} bound {bound[worst]:.3e}")
    assert (bound <= 1e-10).all()
    assert (diff <= bound).all(), [(int(i), c["labels"][i], float(diff[i]), float(bound[i])) for i in np.nonzero(~(diff <= bound))[0]]
    zero = [i for i, l in enumerate(c["labels"]) if l.startswith("omega 0 sigma 0")]
    assert zero and ck.same(d["trial"][zero][:, :4], d["vS"][zero][:, :4])        # exp of no rotation is the identity quaternion, exactly
    ed, em_ = ck.row_diff(runs[0]["echi_trial"][:, None], d["echi_trial"][:, None]), ck.row_spread([r["echi_trial"][:, None] for r in runs])
    print(f"  echi at the trial: largest difference {ed.max():.3e}, largest model spread {em_.max():.3e}")
    assert (ed <= ck.MARGIN * np.maximum(em_, np.median(em_))).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in es.STAGE_CASES if n.startswith("shape-")])
def test_solve(pkg, name):
    """test 7: x behind a real solve, from the device's own S and y.  numpy.linalg has no longdouble solve; the residual is taken in
    longdouble instead, under the bound tests/test_ldlt_panel.py puts on a solution, and x is asked to be the bytes that test asks for"""
    c, d = es.stage_case(name), dump(pkg, name)
    S, y, x = d["S"], d["y"], d["x"]
    n = len(y)
    A = np.tril(S) + np.tril(S, -1).T
    assert d["solve_ok"] == 1 and d["status_trial"][3] == 1.0
    exp = lba_model.ldlt_solve(A, y)
    if c["problem"]["fix_scale"]:                                                 # a scale row is lambda x = 0: the solve itself gives the zero
        assert (x[6::7] == 0.0).all() and (exp[6::7] == 0.0).all()
    res = np.abs(A.astype(np.longdouble) @ x.astype(np.longdouble) - y.astype(np.longdouble)).max()
    print(f"{name}: n {n} residual {float(res):.3e} bound {1e-9 * np.abs(y).max() * len(y):.3e}")
    assert ck.same(d["x"], exp), ck.where(d["x"], exp)
    assert res <= 1e-9 * np.abs(y).max() * len(y)


HOST_LOOP_TAGS = [t for t in es.all_tags() if t not in ("no_edges", "no_iterations")]


@pytest.mark.gpu
def test_one_iteration_leaves_lambda_from_1e_16(pkg):
    """test 9, the mutation "lambda_diag": after ONE iteration with ONE accepted or rejected trial lm_accept / lm_reject leave
    lambda = 1e-16 x a factor in [1 / 3, 2 / 3] after an accepted trial -- from tau x the largest diagonal entry it would be 1e-4 .. 1e-3
    (the model: 2.6e-4 .. 2.1e-3 over these scenes, tools/eg_spread.py --mutations).  In the model every scene has trials == 1 with
    iterations = 1, at every nudge and order."""
    qualify, fix_tags, fix_ok = 0, 0, 0
    for tag in HOST_LOOP_TAGS:
        pr, _ = es.case(tag)
        got = pkg.optimize_essential_graph(pr, iterations=1)
        ok = got["trials"] == 1 and got["n_solve_failed"] == 0 and got["chi2"] < got["chi2_start"]
        print(f"{tag}: trials {got['trials']} failed {got['n_solve_failed']} chi2 {got['chi2_start']:.6g} -> {got['chi2']:.6g} lambda {got['lambda']!r}")
        fix_tags += int(pr["fix_scale"]); fix_ok += int(ok and pr["fix_scale"])
        if ok:
            qualify += 1
            assert 1e-16 * (1.0 / 3.0) <= got["lambda"] <= 1e-16 * (2.0 / 3.0), tag
    print(f"{qualify} of {len(HOST_LOOP_TAGS)} scenes qualify, {fix_ok} of {fix_tags} fix_scale ones")
    assert 2 * fix_ok >= fix_tags and fix_tags >= 8


@pytest.mark.gpu
def test_refusals(pkg):
    """test 10: the problem's refusals are orbx_optimize_essential_graph's (eg_check), then a NULL dump, lambda, and the two capacities;
    none of them sets a device context up"""
    L = pkg.lib()
    base = es.case("5-free")[0]
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    K = len(base["fixed"])
    vS = np.zeros((4200, 8))

    def call(problem=base, null=(), fields=None, lam=0.25, no_dump=False, want=("vS",), x=None, no_problem=False):
        pr, keep = pkg.orbx._eg_problem(problem, "test")
        for k, v in (fields or {}).items():
            setattr(pr, k, v)
        for k in null:
            setattr(pr, k, None)
        d = pkg.orbx.EgStages(**{k: p(vS) for k in want})
        return L.orbx_debug_eg_stages(0, None if no_problem else C.byref(pr), lam, None if x is None else p(x), 1, None if no_dump else C.byref(d))

    before = L.orbx_debug_thread_contexts()
    assert call(no_dump=True) == -1 and "NULL dump" in L.orbx_last_error().decode()
    assert call(no_problem=True) == -1
    for f in ("Tcw", "fixed", "corrected", "noncorrected", "S_corrected", "S_noncorrected", "edge_i", "edge_j", "edge_kind", "Xw", "point_ref"):
        assert call(null=(f,)) == -1, f
    assert call(fields=dict(n_kf=0)) == -1 and call(fields=dict(n_edges=-1)) == -1 and call(fields=dict(n_kf=4097)) == -2
    for key, val in (("edge_i", K), ("edge_j", -1), ("point_ref", K), ("corrected", -2), ("edge_kind", 2)):
        bad = dict(base); bad[key] = base[key].copy(); bad[key][len(bad[key]) // 2] = val
        assert call(bad) == -1, (key, val)
    bad = dict(base); bad["fixed"] = np.zeros(K, np.uint8)
    assert call(bad) == -1 and "exactly one" in L.orbx_last_error().decode()
    for lam in (-1.0, math.nan, math.inf):
        assert call(lam=lam) == -1 and "lambda" in L.orbx_last_error().decode()
    many = dict(base)                                                             # n = 7 x 147 = 1029 > 1024 with S wanted; fine without S
    for k in ("Tcw", "fixed", "corrected", "noncorrected"):
        many[k] = np.concatenate([base[k]] + [base[k][1:2]] * (148 - K))
    assert call(many, want=("vS", "S")) == -2 and "1024" in L.orbx_last_error().decode()
    wide = dict(base)                                                             # 4097 edges with err wanted
    for k in ("edge_i", "edge_j", "edge_kind"):
        wide[k] = np.resize(base[k], 4097)
    assert call(wide, want=("vS", "err")) == -2 and "4096" in L.orbx_last_error().decode()
    assert L.orbx_debug_thread_contexts() == before                              # refused before any device work: nothing was set up
    with pytest.raises(pkg.OrbxError):
        pkg.orbx.eg_stages(base, 0.25, x=np.zeros(3))
    with pytest.raises(pkg.OrbxError):
        pkg.orbx.eg_stages(base, 0.25, want=["nothing"])
    assert call(many) == 0 and call(wide) == 0 and call() == 0                    # the arguments are good
    edgeless = pkg.orbx.eg_stages(es.case("no_edges")[0], 0.25)                   # no iteration runs: the setup's stages alone
    assert set(edgeless) == {"vS", "meas", "xf", "pair", "n_pairs"} and edgeless["n_pairs"] == 0 and len(edgeless["meas"]) == 0
