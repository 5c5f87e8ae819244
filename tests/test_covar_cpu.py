"""CPU tests of tests/covar_restatement.py, the plain-Python MINPACK covar the GPU tests compare against bit for bit.
Yardsticks that share no code with it: a 60-digit inverse of J^T J (tests/golden/covar_vectors.npz, written with mpmath by
tests/golden/make_covar_vectors.py), exact symmetry, the rank rule on a constructed rank-deficient matrix; and the
row / element-parallel formulation the kernels use, which must give the bits of the sequential loops.

The accuracy bound is the textbook one for the inverse of a Gram matrix: max|cov - ref| / max|ref| <= eps cond_2(J)^2
(the pivoted factor R has the singular values of J, so inv(R^T R) carries cond_2(J)^2) -- derived, not tuned."""
import os

import numpy as np
import pytest

import covar_restatement as cr

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = np.finfo(np.float64).eps
NS = (3, 6, 12, 24)


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


@pytest.fixture(scope="module")
def vectors():
    return np.load(os.path.join(HERE, "golden", "covar_vectors.npz"))


def factor(oracle, J):
    """R (n x n, upper) and ipvt of the reference's lmfactor (the CPU oracle), for a Fortran-order m x n J."""
    a, ipvt, rdiag, _ = oracle.lmfactor(np.asfortranarray(J))
    return cr.r_of_lmfactor(a, rdiag), ipvt


def rank5_matrix():
    """50 x 6, column 4 = 2 column 1 (0-based): rank 5."""
    A = np.random.default_rng(6).standard_normal((50, 6))
    A[:, 4] = 2.0 * A[:, 1]
    return A


@pytest.mark.parametrize("n", NS)
def test_accuracy_against_mpmath(oracle, vectors, n):
    J, ref, cond2sq = vectors[f"J_{n}"], vectors[f"ref_{n}"], float(vectors[f"cond2sq_{n}"])
    R, ipvt = factor(oracle, J)
    cov, rank = cr.covar(R, ipvt)
    assert rank == n
    err = np.abs(cov - ref).max() / np.abs(ref).max()
    print(f"n = {n}: err {err:.3e}, bound {EPS * cond2sq:.3e}")
    assert err <= EPS * cond2sq


@pytest.mark.parametrize("n", NS)
def test_exactly_symmetric(oracle, vectors, n):
    R, ipvt = factor(oracle, vectors[f"J_{n}"])
    cov, _ = cr.covar(R, ipvt)
    assert np.array_equal(_bits(cov), _bits(cov.T))


def test_rank_deficient(oracle):
    R, ipvt = factor(oracle, rank5_matrix())
    cov, rank = cr.covar(R, ipvt, 1e-10)
    assert rank == 5
    zero_rows = [i for i in range(6) if not cov[i].any()]
    zero_cols = [j for j in range(6) if not cov[:, j].any()]
    assert zero_rows == zero_cols and len(zero_rows) == 1
    assert zero_rows[0] == ipvt[5] and zero_rows[0] in (1, 4)     # the variable pivoted last is the one dropped
    assert np.array_equal(_bits(cov), _bits(cov.T))
    keep = [i for i in range(6) if i != zero_rows[0]]
    A = rank5_matrix()[:, keep]                                    # the kept 5 x 5 block is the covariance of the reduced fit
    ref = np.linalg.inv(A.T @ A)
    sub = cov[np.ix_(keep, keep)]
    assert np.abs(sub - ref).max() / np.abs(ref).max() <= EPS * np.linalg.cond(A) ** 2


def test_zero_leading_pivot_and_default_tol():
    cov, rank = cr.covar([[0.0, 1.0], [0.0, 2.0]], [0, 1])
    assert rank == 0 and not cov.any()
    cov, rank = cr.covar([[4.0]], [0], tol=0.0)                    # tol <= 0: machine epsilon
    assert rank == 1 and cov[0, 0] == 0.0625
    # the count stops at the first failure: a later large pivot does not come back
    _, rank = cr.covar([[1.0, 0.0, 0.0], [0.0, 1e-20, 0.0], [0.0, 0.0, 1.0]], [0, 1, 2])
    assert rank == 1


@pytest.mark.parametrize("n", NS)
def test_parallel_formulation_same_bits(oracle, vectors, n):
    R, ipvt = factor(oracle, vectors[f"J_{n}"])
    cov, rank = cr.covar(R, ipvt)
    covp, rankp = cr.covar_parallel(R, ipvt)
    assert rank == rankp and np.array_equal(_bits(cov), _bits(covp))


def test_parallel_formulation_same_bits_rank_deficient(oracle):
    R, ipvt = factor(oracle, rank5_matrix())
    for tol in (1e-10, None, 0.5):
        cov, rank = cr.covar(R, ipvt, tol)
        covp, rankp = cr.covar_parallel(R, ipvt, tol)
        assert rank == rankp and np.array_equal(_bits(cov), _bits(covp))


def test_parallel_formulation_random_factors():
    rng = np.random.default_rng(12)
    for n in (1, 2, 5, 9, 17, 40):
        R = np.triu(rng.standard_normal((n, n))) + np.diag(rng.uniform(1.0, 2.0, n))
        ipvt = rng.permutation(n)
        cov, rank = cr.covar(R, ipvt)
        covp, rankp = cr.covar_parallel(R, ipvt)
        assert rank == rankp == n and np.array_equal(_bits(cov), _bits(covp))


def test_fast_form_same_bits(oracle, vectors):
    """covar_fast (numpy slices in the innermost loops; what the GPU tests use at large n) against the plain loops."""
    cases = [factor(oracle, vectors[f"J_{n}"]) + (None,) for n in NS]
    cases += [factor(oracle, rank5_matrix()) + (1e-10,)]
    rng = np.random.default_rng(13)
    for n in (1, 2, 33, 70):
        cases.append((np.triu(rng.standard_normal((n, n))) + np.diag(rng.uniform(1.0, 2.0, n)), rng.permutation(n), None))
    for R, ipvt, tol in cases:
        cov, rank = cr.covar(R, ipvt, tol)
        covf, rankf = cr.covar_fast(R, ipvt, tol)
        assert rank == rankf and np.array_equal(_bits(cov), _bits(covf))


def test_chi2_sigma_and_scaling(oracle, vectors):
    J = vectors["J_6"]
    R, ipvt = factor(oracle, J)
    f = np.random.default_rng(2).standard_normal(J.shape[0]) * 1e-3
    cov0, sig0, rank, c2 = cr.lm_covariance(R, ipvt, f, scaled=False)
    cov1, sig1, _, c2b = cr.lm_covariance(R, ipvt, f, scaled=True)
    assert rank == 6 and c2 == c2b
    assert np.isclose(c2, float(f @ f) / (J.shape[0] - 6), rtol=1e-13)
    assert np.array_equal(_bits(cov1), _bits(cov0 * c2))           # one multiplication per entry
    assert np.array_equal(_bits(sig0), _bits(np.sqrt(np.diag(cov0)))) and np.array_equal(_bits(sig1), _bits(np.sqrt(np.diag(cov1))))
    assert np.isinf(cr.chi2([1.0, 2.0], 2))                         # m == n: the IEEE quotient
