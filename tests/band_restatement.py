"""Plain-numpy restatement of nlh_propagate (include/nonlin_hip.h): the delta method, sd_i = sqrt(J_i C J_i^T), in the
operation order the header makes part of the interface -- one IEEE operation per step, no fused operation.  The yardstick
of tests/test_band_cpu.py and tests/test_gpu_band.py.  The loops over j and k are Python loops; every step is one numpy
operation on the [npoints, m] array of all rows at once (rows never mix)."""
import numpy as np


def variance(J, cov):
    """The double loop: v [npoints, m] before the noise, the clamp and the square root.  J [npoints, n, m] (each point
    column-major m x n, as a Jacobian launcher writes it), cov [npoints, n, n] read by its lower triangle only (cov[p, j, k]
    with k <= j)."""
    J = np.asarray(J, dtype=np.float64)
    cov = np.asarray(cov, dtype=np.float64)
    npoints, n, m = J.shape
    assert cov.shape == (npoints, n, n)
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.zeros((npoints, m))
        for j in range(n):
            s = np.zeros((npoints, m))
            for k in range(j):
                s = s + cov[:, j, k, None] * J[:, k, :]
            s = 2.0 * s
            s = s + cov[:, j, j, None] * J[:, j, :]
            v = v + J[:, j, :] * s
    return v


def finish(v, noise=None):
    """sd from the double loop's v: the noise [npoints] (None: none) added once to every row, the clamp, the square root."""
    with np.errstate(invalid="ignore", over="ignore"):
        if noise is not None:
            v = v + np.asarray(noise, dtype=np.float64)[:, None]
        v = np.where(v < 0.0, 0.0, v)                              # (a NaN compares false and passes through)
        return np.sqrt(v)


def propagate(J, cov, noise=None):
    """sd [npoints, m] of nlh_propagate."""
    return finish(variance(J, cov), noise)


def propagate_longdouble(J, cov, noise=None):
    """The same quantity, J C J^T with the full symmetric matrix, in numpy.longdouble: what the rounding of propagate is
    measured against.  Returns the VARIANCE [npoints, m] (before the clamp and the square root)."""
    Jl = np.asarray(J, dtype=np.longdouble)
    low = np.tril(np.asarray(cov, dtype=np.longdouble))
    Cl = low + np.transpose(np.tril(low, -1), (0, 2, 1))
    v = np.einsum("pji,pjk,pki->pi", Jl, Cl, Jl)
    if noise is not None:
        v = v + np.asarray(noise, dtype=np.longdouble)[:, None]
    return v
