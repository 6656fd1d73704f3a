"""The envelope form of the panel LDL^T (orbx_ldlt_env.hip, orbx_debug_ldlt_solve_envelope) against the dense panel form (form 1 of
orbx_debug_ldlt_solve) on the same matrix with zeros outside the envelope.  In the same row order the envelope solver performs, per stored
entry, the dense solver's operations in the dense solver's order and leaves out only x - (l * 0) * d, so the VALUES are equal and no
tolerance is given: numpy.array_equal.  Bytes can differ in one way only, a -0 that the dense solver's x - (+-0) turns into +0; whether
they were equal is printed.  With first = 0 nothing is left out, and the bytes are those of form 1 and of tests/lba_model.py: ldlt_solve.

The systems are seeded SPD matrices with the stated pattern: M M^T restricted to the pattern, plus n I (checked to factor: the model solves
each).  W is the panel width the library exports; first[] is handed over UNROUNDED and the library rounds it down to W."""
import numpy as np
import pytest

import lba_model as lm

_cache = {}


def rounded(first, W):
    return np.asarray(first) // W * W


def system(n, first, seed):
    """S = (M M^T restricted to first[i] <= j <= i and its mirror image) + n I, b"""
    rng = np.random.Generator(np.random.PCG64(seed))
    M = rng.normal(size=(n, n))
    i, j = np.arange(n)[:, None], np.arange(n)[None, :]
    low = (j >= np.asarray(first)[:, None]) & (j <= i)
    return (M @ M.T) * (low | low.T) + n * np.eye(n), rng.normal(size=n)


def band(n, width):
    return np.maximum(0, np.arange(n) - width)


def cases(W):
    """tag -> (n, first): the band cases of the issue"""
    out = {}
    n = 5 * W + 3
    out["band"] = (n, band(n, 10))
    out["wide_band"] = (300, band(300, 100))                                   # more than 64 active rows a panel: two row tiles, three trailing tiles
    n = 7 * W + 5
    f = band(n, 20)
    f[100] = 5
    f[-3:] = 0                                                                 # far-reaching rows, first[] not monotone: active lists with gaps
    out["far_rows"] = (n, f)
    n = 5 * W + 3
    f = band(n, 10)
    iso = 2 * W
    f[iso] = iso                                                               # the vertex without an edge: a row of its diagonal entry alone ...
    f[iso + 1:] = np.maximum(f[iso + 1:], iso + 1)                             # ... that no later row reaches
    out["isolated_row"] = (n, f)
    return out


def world(pkg, tag):
    """a case's system and form 1's answer on it, computed once and left alone"""
    W = pkg.orbx.ldlt_panel_width()
    if tag not in _cache:
        n, first = cases(W)[tag]
        S, b = system(n, first, 9300 + sorted(cases(W)).index(tag))
        S.setflags(write=False); b.setflags(write=False)
        x1, ok1 = pkg.orbx.ldlt_solve(S, b, 1)
        assert ok1, tag
        _cache[tag] = (n, first, S, b, x1)
    return _cache[tag]


def test_the_systems_factor():
    """not a GPU test: every pattern-restricted matrix used below is positive definite in the solver's own arithmetic"""
    W = 32
    for k, (tag, (n, first)) in enumerate(sorted(cases(W).items())):
        S, b = system(n, first, 9300 + k)
        x = lm.ldlt_solve(S, b)
        assert x is not None and np.abs(S @ x - b).max() <= 1e-9 * np.abs(b).max() * n, tag
        i, j = np.nonzero(np.tril(S))
        assert (j >= rounded(first, W)[i]).all() and (j >= np.asarray(first)[i]).all(), tag


@pytest.mark.gpu
def test_a_full_envelope_is_the_dense_solver(pkg):
    W = pkg.orbx.ldlt_panel_width()
    for n in (1, W - 1, W, W + 1, 2 * W + 1, 5 * W + 3):
        S, b = system(n, np.zeros(n, int), 9200 + n)
        exp = lm.ldlt_solve(S, b)
        x1, ok1 = pkg.orbx.ldlt_solve(S, b, 1)
        xe, oke = pkg.orbx.ldlt_solve_envelope(S, b, np.zeros(n, np.int32))
        assert ok1 and oke, n
        assert xe.tobytes() == x1.tobytes(), (n, np.abs(xe - x1).max())
        assert xe.tobytes() == exp.tobytes(), (n, np.abs(xe - exp).max())


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["band", "wide_band", "far_rows", "isolated_row"])
def test_equals_the_dense_solver_on_the_same_matrix(pkg, tag):
    n, first, S, b, x1 = world(pkg, tag)
    xe, oke = pkg.orbx.ldlt_solve_envelope(S, b, first)
    print(f"{tag}: n {n} bytes equal {xe.tobytes() == x1.tobytes()}")
    assert oke
    assert np.array_equal(xe, x1), np.abs(xe - x1).max()
    if tag == "isolated_row":
        iso = 2 * pkg.orbx.ldlt_panel_width()
        assert xe[iso] == b[iso] / S[iso, iso]


@pytest.mark.gpu
def test_nothing_outside_the_envelope_is_read(pkg):
    n, first, S, b, x1 = world(pkg, "far_rows")
    W = pkg.orbx.ldlt_panel_width()
    P = S.copy()
    j = np.arange(n)[None, :]
    P[j < rounded(first, W)[:, None]] = np.nan                                 # every entry left of the rounded first[i]
    P[np.triu_indices(n, 1)] = np.nan                                          # and everything above the diagonal
    assert np.isnan(P).sum() > n
    xe, oke = pkg.orbx.ldlt_solve_envelope(P, b, first)
    assert oke and np.array_equal(xe, x1)


@pytest.mark.gpu
def test_pivot_not_positive(pkg):
    n, first, S0, b, x1 = world(pkg, "band")
    W = pkg.orbx.ldlt_panel_width()
    for j in (3, 2 * W + 5, n - 1):                                            # the first diagonal block, a later panel, the last column
        S = S0.copy()
        S[j, j] = -1.0
        assert lm.ldlt_solve(S, b) is None
        x0 = np.arange(n) + 7.0
        x, ok = pkg.orbx.ldlt_solve_envelope(S, b, first, x0=x0)
        assert not ok and x.tobytes() == x0.tobytes(), j
        S[j, j] = 0.0                                                          # a column of zeros in front of it: the pivot is exactly 0
        S[j, :j] = 0.0
        x, ok = pkg.orbx.ldlt_solve_envelope(S, b, first, x0=np.ones(n))
        assert not ok and (x == 1.0).all(), j
    S = S0.copy()
    S[0, 0] = np.nan
    x, ok = pkg.orbx.ldlt_solve_envelope(S, b, first, x0=np.ones(n))
    assert not ok and (x == 1.0).all()
    xe, oke = pkg.orbx.ldlt_solve_envelope(S0, b, first)                       # and the next good call is not disturbed by the failed ones
    assert oke and np.array_equal(xe, x1)
