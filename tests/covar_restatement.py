"""Plain-Python restatement of MINPACK's covar (0-based) and of what nlh_lm_covariance* add to it: the yardstick of
tests/test_gpu_covar.py, itself held to mpmath, symmetry and rank handling in tests/test_covar_cpu.py.

Python floats are IEEE doubles and `a - t * b` is a multiply followed by a subtraction (no fused operation), so these loops
ARE the operation order the kernels of nonlin_amd/csrc/nlh_kernels_covar.h must reproduce bit for bit.

covar(r, ipvt, tol)            the textbook sequential loops, statement for statement
covar_parallel(r, ipvt, tol)   the row / element formulation the workgroup kernels use (a chain per row of the inverse, a
                               chain per element of the product): the same bits, which test_covar_cpu.py asserts
covar_fast(r, ipvt, tol)       the sequential loops with the innermost one as a numpy slice operation (elementwise IEEE
                               multiply, then subtract / add: the same bits, asserted in test_covar_cpu.py) -- what the GPU
                               tests use at n in the hundreds, where the plain loops take minutes
chi2 / lm_covariance           reduced chi-square, scaling, standard errors
"""
import math

import numpy as np

EPS = 2.220446049250313e-16


def _tol(tol):
    return tol if (tol is not None and tol > 0.0) else EPS


def covar(r, ipvt, tol=None):
    """r: n x n array-like, r[i][j] = R(i, j) for i <= j (the rest is ignored); ipvt: 0-based permutation.
    Returns (cov as a float64 [n, n] array, rank)."""
    n = len(ipvt)
    r = [[float(r[i][j]) for j in range(n)] for i in range(n)]
    ipvt = [int(v) for v in ipvt]
    tol = _tol(tol)
    # the inverse of r in its full upper triangle
    tolr = tol * abs(r[0][0])
    l = 0
    for k in range(n):
        if abs(r[k][k]) <= tolr:
            break
        r[k][k] = 1.0 / r[k][k]
        for j in range(k):
            temp = r[k][k] * r[j][k]
            r[j][k] = 0.0
            for i in range(j + 1):
                r[i][k] = r[i][k] - temp * r[i][j]
        l = k + 1
    # the full upper triangle of the inverse of (r transpose) r
    for k in range(l):
        for j in range(k):
            temp = r[j][k]
            for i in range(j + 1):
                r[i][j] = r[i][j] + temp * r[i][k]
        temp = r[k][k]
        for i in range(k + 1):
            r[i][k] = temp * r[i][k]
    # the full lower triangle of the covariance matrix in the strict lower triangle of r and in wa
    wa = [0.0] * n
    for j in range(n):
        jj = ipvt[j]
        sing = j >= l
        for i in range(j + 1):
            if sing:
                r[i][j] = 0.0
            ii = ipvt[i]
            if ii > jj:
                r[ii][jj] = r[i][j]
            if ii < jj:
                r[jj][ii] = r[i][j]
        wa[jj] = r[j][j]
    # symmetrize
    for j in range(n):
        for i in range(j + 1):
            r[i][j] = r[j][i]
        r[j][j] = wa[j]
    return np.array(r, dtype=np.float64).reshape(n, n), l


def covar_parallel(r, ipvt, tol=None):
    """The same result from independent chains: row i of the inverse from row i's earlier columns and the original r;
    element (i, j) of the product from rows i and j of the inverse."""
    n = len(ipvt)
    r = [[float(r[i][j]) for j in range(n)] for i in range(n)]
    ipvt = [int(v) for v in ipvt]
    tol = _tol(tol)
    tolr = tol * abs(r[0][0])
    l = 0
    for k in range(n):
        if abs(r[k][k]) <= tolr:
            break
        l = k + 1
    inv = [[0.0] * n for _ in range(n)]
    for i in range(l):                                  # "a thread per row"
        for k in range(i, l):
            d = 1.0 / r[k][k]
            if k == i:
                inv[i][k] = d
                continue
            acc = 0.0
            for j in range(i, k):
                t = d * r[j][k]
                acc = acc - t * inv[i][j]
            inv[i][k] = acc
    cov = np.zeros((n, n))
    for j in range(n):                                  # "a thread per element"
        for i in range(j + 1):
            c = 0.0
            if j < l:
                c = inv[j][j] * inv[i][j]
                for k in range(j + 1, l):
                    c = c + inv[j][k] * inv[i][k]
            cov[ipvt[i], ipvt[j]] = c
            cov[ipvt[j], ipvt[i]] = c
    return cov, l


def covar_fast(r, ipvt, tol=None):
    """covar with its innermost loops over i as numpy slices (no reduction: each element still sees one multiply and one
    add or subtract per step, in the same order)."""
    n = len(ipvt)
    r = np.array(r, dtype=np.float64).reshape(n, n).copy()
    ipvt = np.asarray(ipvt, dtype=np.int64)
    tol = _tol(tol)
    tolr = tol * abs(float(r[0, 0]))
    l = 0
    for k in range(n):
        if abs(float(r[k, k])) <= tolr:
            break
        r[k, k] = 1.0 / r[k, k]
        for j in range(k):
            temp = r[k, k] * r[j, k]
            r[j, k] = 0.0
            r[:j + 1, k] = r[:j + 1, k] - temp * r[:j + 1, j]
        l = k + 1
    for k in range(l):
        for j in range(k):
            temp = r[j, k]
            r[:j + 1, j] = r[:j + 1, j] + temp * r[:j + 1, k]
        temp = r[k, k]
        r[:k + 1, k] = temp * r[:k + 1, k]
    cov = np.zeros((n, n))
    for j in range(l):
        ii, jj = ipvt[:j + 1], ipvt[j]
        cov[ii, jj] = r[:j + 1, j]
        cov[jj, ii] = r[:j + 1, j]
    return cov, l


def chi2(fvec, n):
    """(sum of f_i^2, i ascending, plain sequential sum) / (m - n); m == n gives the IEEE quotient by zero."""
    s = 0.0
    for v in fvec:
        v = float(v)
        s = s + v * v
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.float64(s) / np.float64(len(fvec) - n))


def lm_covariance(r, ipvt, fvec, scaled=True, tol=None, parallel=False, fast=False):
    """What nlh_lm_covariance* return from the factor (r, ipvt) of the Jacobian and the residuals fvec:
    (cov, sigma, rank, chi2)."""
    n = len(ipvt)
    cov, rank = (covar_fast if fast else covar_parallel if parallel else covar)(r, ipvt, tol)
    c2 = chi2(fvec, n)
    if scaled:
        cov = np.array([[float(cov[i, j]) * c2 for j in range(n)] for i in range(n)], dtype=np.float64).reshape(n, n)
    sigma = np.array([math.sqrt(float(cov[i, i])) for i in range(n)], dtype=np.float64)
    return cov, sigma, rank, c2


def r_of_lmfactor(a_out, rdiag):
    """The n x n factor covar reads, from oracle.lmfactor's outputs (R strictly above the diagonal of a_out, rdiag)."""
    n = len(rdiag)
    r = np.triu(np.asarray(a_out)[:n, :n], 1)
    r[np.arange(n), np.arange(n)] = rdiag
    return r
