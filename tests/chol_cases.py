"""What the Cholesky tests (tests/test_gpu_chol_natural.py, tests/test_chol_cases_cpu.py) share: seeded inputs whose
factor spans six decades, two numpy.longdouble references (natural order, greedy pivoting) and the three assertion helpers.

Layout as everywhere: a problem's matrices are column-major, G[p, c, r] = G(r, c); a factor comes back in the upper
triangle, R[p, c, r] = R(r, c) for r <= c.  The helpers below take plain row-major numpy views, R[r, c] = R(r, c).

The backward identity.  For a computed Cholesky factor Higham (Accuracy and Stability of Numerical Algorithms, 2nd ed.,
Theorem 10.3) gives |R^T R - G| <= gamma_{n+1} |R|^T |R| entry by entry; its proof bounds each inner product
r_ij = (a_ij - sum_k r_ki r_kj) / r_ii for any order of the sum and also holds with fused multiply-adds, hence for the
MFMA tiles.  The natural-order kernels do not divide by r_ii: they multiply by a reciprocal r from sqrt_rsqrt whose error
is at most E_R ulp (derived in tests/test_gpu_chol_natural.py), while the stored diagonal s is sqrt rounded once more
(within 1/2 ulp but for near-ties).  With t the numerator, the stored r_ij = t r (1 + rho) and the stored r_ii = s give
r_ii r_ij = t (1 + e_s)(1 + e_r)(1 + rho).  In units of u = 2^-53 an error of e ulp is at most 2 e u relative: the
reciprocal costs at most 2 E_R u, the diagonal 1 u and the multiplication 1 u on top of the theorem's n + 1:
c = 2 E_R + 2, gamma = (n + 1 + c) u.
The longdouble products that stand for the exact ones are themselves off by at most n 2^-64 |R|^T|R| = (n / 2048) u
|R|^T|R|, half a unit at n = 1109, against bounds of n + 9 units."""
import functools

import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the references need an extended-precision long double"
U = 2.0 ** -53
E_R = 3                                 # ulp bound of sqrt_rsqrt's reciprocal against the correctly rounded 1 / sqrt(x)
C_RECIP = 2 * E_R + 2
NB = 16                                 # panel width of the blocked kernels


def gamma_units(n, c=C_RECIP):
    """The bound of the backward identities in units of 2^-53 |R|^T |R|."""
    return n + 1 + c


# ---- inputs -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _problem(n, seed, m):
    rng = np.random.default_rng([20240611, n, seed, m])
    J = rng.standard_normal((m, n)) * np.exp(rng.uniform(-3.0, 3.0, n))
    f = rng.standard_normal(m)
    for a in (J, f):
        a.setflags(write=False)
    return J, f


def jac(n, seed, m=None):
    """J (m-by-n, m = n + 40 unless given) with its columns scaled by exp(uniform(-3, 3)), and f (m): the entries of R
    span six decades, so a dropped term cannot hide under a uniform scale."""
    return _problem(n, seed, n + 40 if m is None else m)


def wellcond_jac(m, n, seed):
    """J (m-by-n) = Q1 diag(sigma) Q2^T with sigma in [1, 2] and columns scaled by exp(uniform(-0.5, 0.5)), and f (m):
    cond(J) < 6, so the Cholesky factor of J^T J and lmfactor's R agree to a few hundred roundings, and the column
    norms are distinct, so both pick the same pivot order."""
    rng = np.random.default_rng([20240612, m, n, seed])
    Q1, _ = np.linalg.qr(rng.standard_normal((m, n)))
    Q2, _ = np.linalg.qr(rng.standard_normal((n, n)))
    J = (Q1 * rng.uniform(1.0, 2.0, n)) @ Q2.T * np.exp(rng.uniform(-0.5, 0.5, n))
    return np.ascontiguousarray(J), rng.standard_normal(m)


def gram_of(J, f):
    """G = J^T J symmetrised, g = J^T f, in float64: the identities are stated for the G the kernel is given."""
    G = J.T @ J
    G = 0.5 * (G + G.T)
    return np.ascontiguousarray(G), J.T @ f


@functools.lru_cache(maxsize=None)
def problem(n, seed):
    G, g = gram_of(*jac(n, seed))
    G.setflags(write=False)
    g.setflags(write=False)
    return G, g


def batch(n, nprob):
    """nprob distinct problems of size n as (G [nprob, n, n], g [nprob, n]): three seeded ones, every further one a
    symmetric cyclic shift of one of them -- another positive definite matrix with another factor, for the price of a
    copy (32 seeded Gram products at n = 1109 would cost seconds)."""
    Gs, gs = [], []
    for p in range(nprob):
        G, g = problem(n, p % 3)
        if p >= 3:
            sh = (7 * p) % n
            G, g = np.roll(np.roll(G, sh, axis=0), sh, axis=1), np.roll(g, sh)
        Gs.append(G)
        gs.append(g)
    return np.stack(Gs), np.stack(gs)


def singular_problem(n, seed, j0, j1):
    """Column j0 of J an exact copy of column j1 < j0: G is exactly singular at j0 (its rows j0 and j1 are the same bits)."""
    J, f = jac(n, seed)
    J = J.copy()
    J[:, j0] = J[:, j1]
    return gram_of(J, f)


# ---- references ---------------------------------------------------------------------------------------------------------
def ref_chol(G, pivot_tol=None):
    """Right-looking Cholesky in longdouble.  Returns (R upper, d) with d[j] the Schur diagonal met at column j.  With a
    pivot_tol it stops at the first column whose d[j] is not above pivot_tol * G[j, j] (or not positive) and returns
    (R, d, info) with info that 1-based column (0: none) -- the kernels' rule with acnorm^2 = G[j, j]."""
    n = G.shape[0]
    A = np.array(G, dtype=LD)
    R = np.zeros((n, n), dtype=LD)
    d = np.zeros(n, dtype=LD)
    info = 0
    for j in range(n):
        d[j] = A[j, j]
        if pivot_tol is not None and (not d[j] > LD(pivot_tol) * LD(G[j, j]) or not d[j] > 0):
            info = j + 1
            break
        R[j, j] = np.sqrt(d[j])
        R[j, j + 1:] = A[j, j + 1:] / R[j, j]
        A[j + 1:, j + 1:] -= np.outer(R[j, j + 1:], R[j, j + 1:])
    return (R, d) if pivot_tol is None else (R, d, info)


def ref_chol_pivoted(G):
    """Greedy-pivoted Cholesky in longdouble: the first maximum of the remaining Schur diagonal (lmfactor's "largest
    remaining column norm").  Returns (perm 0-based, R upper of P^T G P, margin) with margin the smallest relative lead
    (d_max - d_second) / d_max of a winner over the runner-up."""
    n = G.shape[0]
    A = np.array(G, dtype=LD)
    perm = np.arange(n)
    R = np.zeros((n, n), dtype=LD)
    margin = np.inf
    for j in range(n):
        dd = np.diagonal(A)[j:]
        q = j + int(np.argmax(dd))                    # argmax returns the first maximum
        if n - j > 1:
            second = np.max(np.delete(dd, q - j))
            margin = min(margin, float((dd[q - j] - second) / dd[q - j]))
        if q != j:
            A[[j, q], :] = A[[q, j], :]
            A[:, [j, q]] = A[:, [q, j]]
            R[:, [j, q]] = R[:, [q, j]]
            perm[[j, q]] = perm[[q, j]]
        R[j, j] = np.sqrt(A[j, j])
        R[j, j + 1:] = A[j, j + 1:] / R[j, j]
        A[j + 1:, j + 1:] -= np.outer(R[j, j + 1:], R[j, j + 1:])
    return perm, R, margin


def rtr_upper(R, B=64):
    """The upper triangle of R^T R for an upper-triangular R, in R's precision, touching only the blocks that are not
    zero by structure (a sixth of the full product's work)."""
    n = R.shape[0]
    out = np.zeros((n, n), dtype=R.dtype)
    for j0 in range(0, n, B):
        j1 = min(n, j0 + B)
        for i0 in range(0, j1, B):
            i1 = min(n, i0 + B)
            out[i0:i1, j0:j1] = R[:i1, i0:i1].T @ R[:i1, j0:j1]
    return np.triu(out)


# ---- the three helpers ------------------------------------------------------------------------------------------------------
def _ratio(diff, scale):
    """max |diff| / (U scale); an entry with scale == 0 must have diff == 0."""
    diff, scale = np.abs(diff), np.asarray(scale, dtype=LD)
    zero = scale == 0
    if np.any(diff[zero] != 0):
        return np.inf
    return float(np.max(np.where(zero, LD(0), diff / np.where(zero, LD(1), scale)))) / U


def backward_ratio(R, G):
    """max over the upper triangle of |R^T R - G| / (2^-53 |R|^T |R|); R float64 upper triangular."""
    n = R.shape[0]
    Ru = np.triu(R)
    iu = np.triu_indices(n)
    prod = rtr_upper(Ru.astype(LD))
    absprod = np.abs(Ru).T @ np.abs(Ru)                 # the scale: float64 is ample
    return _ratio((prod - G.astype(LD))[iu], absprod[iu])


def gradient_ratio(R, qtf, g):
    """max |R^T qtf - g| / (2^-53 |R|^T |qtf|)."""
    Rl = np.triu(R).astype(LD)
    return _ratio(Rl.T @ qtf.astype(LD) - g.astype(LD), np.abs(Rl).T @ np.abs(qtf.astype(LD)))


def assert_backward(R, G, c=C_RECIP, what=""):
    """|R^T R - G| <= gamma |R|^T |R| entry by entry, gamma = (n + 1 + c) 2^-53.  Returns the largest ratio in units of
    2^-53 |R|^T |R|."""
    r = backward_ratio(R, G)
    assert r <= gamma_units(R.shape[0], c), (what, "R^T R - G", r, gamma_units(R.shape[0], c))
    return r


def assert_gradient(R, qtf, g, c=C_RECIP, what=""):
    """|R^T qtf - g| <= gamma |R|^T |qtf| entry by entry.  Returns the largest ratio."""
    r = gradient_ratio(R, qtf, g)
    assert r <= gamma_units(R.shape[0], c), (what, "R^T qtf - g", r, gamma_units(R.shape[0], c))
    return r


def assert_structure(Rfull, G, acnorm, ipvt, what=""):
    """Rfull[r, c] is the kernel's whole output matrix: its strict lower triangle is G's bit for bit (the kernels write
    only r <= c), acnorm == sqrt(max(diag G, 0)) bit for bit, ipvt is the identity."""
    n = G.shape[0]
    il = np.tril_indices(n, -1)
    assert np.array_equal(Rfull[il].view(np.int64), G[il].view(np.int64)), (what, "strict lower triangle")
    want = np.sqrt(np.maximum(np.diagonal(G), 0.0))
    assert np.array_equal(np.asarray(acnorm).view(np.int64), want.view(np.int64)), (what, "acnorm")
    assert np.array_equal(np.asarray(ipvt), np.arange(n)), (what, "ipvt")


def check_natural(Rfull, qtf, acnorm, ipvt, G, g, what=""):
    """All three helpers on one problem's output of a natural-order kernel.  Returns (backward ratio, gradient ratio)."""
    assert_structure(Rfull, G, acnorm, ipvt, what)
    return assert_backward(Rfull, G, what=what), assert_gradient(Rfull, qtf, g, what=what)


# ---- a float64 model of the blocked kernels, with the faults the helpers are for -------------------------------------
def blocked_chol(G, g, fault=None):
    """Right-looking blocked Cholesky (panels of NB columns, trailing update in NB x NB tiles) in float64, the gradient as
    column n.  fault = ("tile", step, tc, tr): that step leaves trailing tile (tr, tc) un-updated;
    fault = ("term", step, k): that step's update of the LAST block (a partial one if n % NB != 0) misses panel row k.
    Returns (R upper, qtf)."""
    n = G.shape[0]
    A = np.triu(np.array(G, dtype=np.float64))
    y = np.array(g, dtype=np.float64)
    for step, jb in enumerate(range(0, n, NB)):
        nbk = min(NB, n - jb)
        t0 = jb + nbk
        for j in range(jb, t0):                         # diagonal block and block row, column n = the gradient
            with np.errstate(invalid="ignore"):         # (a fault may leave a negative pivot: NaN, which fails every bound)
                A[j, j] = np.sqrt(A[j, j])
            A[j, j + 1:] /= A[j, j]
            y[j] /= A[j, j]
            A[j + 1:t0, j + 1:] -= np.outer(A[j, j + 1:t0], A[j, j + 1:])
            y[j + 1:t0] -= A[j, j + 1:t0] * y[j]
        P = A[jb:t0, t0:]
        nt = (n - t0 + NB - 1) // NB
        for tc in range(nt):
            for tr in range(tc + 1):
                if fault and fault[0] == "tile" and fault[1:] == (step, tc, tr):
                    continue
                rows = slice(tr * NB, min((tr + 1) * NB, n - t0))
                cols = slice(tc * NB, min((tc + 1) * NB, n - t0))
                Pr = P[:, rows]
                if fault and fault[0] == "term" and fault[1] == step and tc == nt - 1:
                    Pr = Pr.copy()
                    Pr[fault[2], :] = 0.0
                T = A[t0:, t0:][rows, cols] - Pr.T @ P[:, cols]
                A[t0:, t0:][rows, cols] = np.triu(T) if tr == tc else T
        y[t0:] -= P.T @ y[jb:t0]
    return np.triu(A), y
