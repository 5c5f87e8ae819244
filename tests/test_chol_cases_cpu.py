"""The assertion helpers of tests/chol_cases.py on factors whose quality is known: LAPACK's own Cholesky factor must pass
them far inside the bound, and two faulty factors of the kind the helpers are for -- one 16 x 16 trailing tile left
un-updated, one k term missing from the update of a partial last block -- must fail them.  Host code: needs no GPU.

Above n = 600 only the longdouble product (the backward identity) is formed, not the longdouble factorisation."""
import numpy as np
import pytest

import chol_cases as CC


def _lapack(G, g):
    L = np.linalg.cholesky(G)
    R = np.ascontiguousarray(L.T)
    qtf = np.zeros_like(g)                              # R^T qtf = g by forward substitution
    for j in range(len(g)):
        qtf[j] = (g[j] - R[:j, j] @ qtf[:j]) / R[j, j]
    return R, qtf


@pytest.mark.parametrize("n", [16, 193, 529, 1109])
def test_lapack_factor_passes_the_helpers(n):
    G, g = CC.problem(n, 0)
    R, qtf = _lapack(G, g)
    # the helpers take the kernel's whole output matrix: the factor above the diagonal, G below it
    full = np.triu(R) + np.tril(G, -1)
    rb, rg = CC.check_natural(full, qtf, np.sqrt(np.diagonal(G)), np.arange(n), G, g, what=f"lapack n={n}")
    print(f"n={n}: backward ratio {rb:.2f}, gradient ratio {rg:.2f} (units of 2^-53 |R|^T|R|), bound {CC.gamma_units(n)}")
    assert rb <= 10.0                                   # (the reference sits far inside the bound: 2.5 - 7.1 measured)
    d = np.abs(np.diagonal(R))
    assert d.max() / d.min() > 50.0                     # the scaled columns do spread the factor


@pytest.mark.parametrize("n", [16, 193, 529])
def test_longdouble_references_pass_the_helpers(n):
    """The two longdouble references, rounded to float64, against the same identities (an entry of R rounded once:
    half a unit per factor, far inside the bound); the greedy order is a permutation led by the largest diagonal."""
    G, g = CC.problem(n, 1)
    R, d = CC.ref_chol(G)
    assert (d > 0).all()
    assert CC.backward_ratio(R.astype(np.float64), G) <= 4.0
    perm, Rp, margin = CC.ref_chol_pivoted(G)
    assert sorted(perm) == list(range(n)) and perm[0] == int(np.argmax(np.diagonal(G)))
    assert margin > 0
    assert CC.backward_ratio(Rp.astype(np.float64), G[np.ix_(perm, perm)]) <= 4.0
    dp = np.diagonal(Rp)
    assert (dp[:-1] >= dp[1:]).all()                    # greedy pivoting: a non-increasing diagonal


def test_reference_names_the_singular_column():
    G, g = CC.singular_problem(40, 2, 33, 7)
    R, d, info = CC.ref_chol(G, pivot_tol=1e-8)
    assert info == 34
    assert (d[:33] > 1e-3 * np.diagonal(G)[:33]).all()
    assert CC.ref_chol(CC.problem(40, 2)[0], pivot_tol=1e-8)[2] == 0


@pytest.mark.parametrize("n", [193, 200])
def test_helpers_see_the_faults_they_are_for(n):
    """n = 193: twelve full blocks and a last block of one column; n = 200: a last block of eight."""
    G, g = CC.problem(n, 3)
    R, qtf = CC.blocked_chol(G, g)
    full = np.triu(R) + np.tril(G, -1)
    CC.check_natural(full, qtf, np.sqrt(np.diagonal(G)), np.arange(n), G, g, what="blocked model")
    # one tile of one step left un-updated: off the diagonal, on it, and the corner tile of the partial block
    for fault in (("tile", 2, 5, 3), ("tile", 0, 4, 4), ("tile", 6, (n - 7 * 16 + 15) // 16 - 1, 0)):
        Rf, qf = CC.blocked_chol(G, g, fault)
        with pytest.raises(AssertionError):
            CC.assert_backward(Rf, G, what=str(fault))
    # a single k term missing from the update of the partial last block
    for fault in (("term", 0, 15), ("term", 9, 0), ("term", (n - 1) // 16 - 1, 7)):
        Rf, qf = CC.blocked_chol(G, g, fault)
        with pytest.raises(AssertionError):
            CC.assert_backward(Rf, G, what=str(fault))
    # a gradient column that misses one step's update
    qbad = qtf.copy()
    qbad[n - 1] += R[5, n - 1] * qtf[5] / R[n - 1, n - 1]
    with pytest.raises(AssertionError):
        CC.assert_gradient(R, qbad, g)
    # and the structure helper: a write below the diagonal, a wrong acnorm bit, a pivot order
    bad = full.copy()
    bad[n - 1, 0] = np.nextafter(bad[n - 1, 0], np.inf)
    with pytest.raises(AssertionError):
        CC.assert_structure(bad, G, np.sqrt(np.diagonal(G)), np.arange(n))
    acn = np.sqrt(np.diagonal(G))
    acn[3] = np.nextafter(acn[3], 0.0)
    with pytest.raises(AssertionError):
        CC.assert_structure(full, G, acn, np.arange(n))
    with pytest.raises(AssertionError):
        CC.assert_structure(full, G, np.sqrt(np.diagonal(G)), np.arange(n)[::-1])
