"""The panel form of the bundle adjustments' dense LDL^T (orbx_ldlt.hip, form 1 of orbx_debug_ldlt_solve) against the one-workgroup kernel
k_lba_solve (form 0) and against tests/lba_model.py: ldlt_solve, BYTE FOR BYTE: a blocked right-looking factorisation applies a panel's
columns to every entry in ascending order with the same three unfused operations, so no tolerance is needed or given.  The systems are
seeded SPD matrices M M^T + n I.  The sizes sit round the panel width W the library exports: one column, a panel short of one column, one
panel, one column more (the first row below a panel, the first trailing tile), two panels and a column, 5 W + 3 (several trailing tiles,
a short last panel), 1536 (the last size the one-workgroup kernel takes) and 1542 (the first it does not)."""
import numpy as np
import pytest

import lba_model as lm
import lba_scene as ls

_cache = {}


def system(n):
    rng = np.random.Generator(np.random.PCG64(9000 + n))
    M = rng.normal(size=(n, n))
    return M @ M.T + n * np.eye(n), rng.normal(size=n)


def sizes(W):
    return [1, W - 1, W, W + 1, 2 * W + 1, 5 * W + 3]


@pytest.mark.gpu
def test_panels_equal_one_workgroup_and_the_model(pkg):
    W = pkg.orbx.ldlt_panel_width()
    assert W >= 2
    for n in sizes(W):
        S, b = system(n)
        exp = lm.ldlt_solve(S, b)
        x0, ok0 = pkg.orbx.ldlt_solve(S, b, 0)
        x1, ok1 = pkg.orbx.ldlt_solve(S, b, 1)
        assert ok0 and ok1, n
        assert np.abs(S @ exp - b).max() <= 1e-9 * np.abs(b).max() * n        # the model solves the system at all
        assert x1.tobytes() == x0.tobytes(), (n, np.abs(x1 - x0).max())
        assert x1.tobytes() == exp.tobytes(), (n, np.abs(x1 - exp).max())


@pytest.mark.gpu
def test_largest_size_of_the_one_workgroup_kernel(pkg):
    S, b = system(1536)
    x0, ok0 = pkg.orbx.ldlt_solve(S, b, 0)
    x1, ok1 = pkg.orbx.ldlt_solve(S, b, 1)
    assert ok0 and ok1 and x1.tobytes() == x0.tobytes()
    with pytest.raises(pkg.OrbxError):
        pkg.orbx.ldlt_solve(*system(1537), 0)


@pytest.mark.gpu
def test_beyond_the_one_workgroup_kernel(pkg):
    S, b = system(1542)
    exp = lm.ldlt_solve(S, b)
    x1, ok1 = pkg.orbx.ldlt_solve(S, b, 1)
    assert ok1 and x1.tobytes() == exp.tobytes(), np.abs(x1 - exp).max()


@pytest.mark.gpu
def test_pivot_not_positive(pkg):
    W = pkg.orbx.ldlt_panel_width()
    n = 5 * W + 3
    for j in (3, 2 * W + 5, n - 1):                                            # the first diagonal block, a later panel, the last column
        S, b = system(n)
        S[j, j] = -1.0
        assert lm.ldlt_solve(S, b) is None
        for form in (0, 1):
            x0 = np.arange(n) + 7.0
            x, ok = pkg.orbx.ldlt_solve(S, b, form, x0=x0)
            assert not ok and x.tobytes() == x0.tobytes(), (j, form)
        S[j, j] = 0.0                                                          # a column of zeros in front of it: the pivot is exactly 0
        S[j, :j] = 0.0
        x, ok = pkg.orbx.ldlt_solve(S, b, 1, x0=np.ones(n))
        assert not ok and (x == 1.0).all(), j
    S, b = system(n)
    S[0, 0] = np.nan
    assert not pkg.orbx.ldlt_solve(S, b, 1)[1] and not pkg.orbx.ldlt_solve(S, b, 0)[1]


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["1-1-8-mono", "11-3-200-mixed", "43-6-600-stereo", "all_fixed"])
def test_local_bundle_adjustment_is_the_same_bytes_with_panels(pkg, tag):
    if "scenes" not in _cache:
        _cache["scenes"] = dict(ls.all_scenes())
    pr = _cache["scenes"][tag]["problem"]
    base = pkg.local_bundle_adjustment(pr)
    pkg.orbx.set_lba_solver(1)
    try:
        got = pkg.local_bundle_adjustment(pr)
    finally:
        pkg.orbx.set_lba_solver(0)
    assert base.keys() == got.keys()
    for k in base:                                                             # every output, the double ones and the report included
        assert np.asarray(got[k]).tobytes() == np.asarray(base[k]).tobytes(), k
    assert np.asarray(pkg.local_bundle_adjustment(pr)["pose"]).tobytes() == base["pose"].tobytes()
    with pytest.raises(pkg.OrbxError):
        pkg.orbx.set_lba_solver(2)
