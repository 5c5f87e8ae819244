"""Global fits (include/nonlin_hip.h: nlh_group_*) restated in numpy: the order of the outer unknowns, gather, expand and the
scattered Jacobian.  Nothing here computes: every step copies values or writes +0.0, so the device kernels reproduce every
function bit for bit.  A group is the tuple (N, sidx, lidx, G) that tables() builds on its own from (nfull, shared, nsets),
which is what the tests hold the library's nlh_group_index to.  Test infrastructure, not part of the product."""
import numpy as np


def tables(nfull, shared=(), nsets=1):
    """(N, sidx, lidx, G): the shared and the local inner indices, each ascending."""
    sidx = np.array(sorted(int(k) for k in shared), dtype=np.int32)
    lidx = np.array([k for k in range(nfull) if k not in set(sidx.tolist())], dtype=np.int32)
    return int(nfull), sidx, lidx, int(nsets)


def nouter(T):
    N, sidx, lidx, G = T
    return len(sidx) + G * len(lidx)


def index(T, g, k):
    """The outer unknown of inner parameter k of data set g: the shared parameters first, in ascending inner index, then per
    data set its local parameters in ascending inner index."""
    N, sidx, lidx, G = T
    if k in sidx:
        return int(np.flatnonzero(sidx == k)[0])
    return len(sidx) + g * len(lidx) + int(np.flatnonzero(lidx == k)[0])


def outer_index(T):
    """[G, N] array of index(T, g, k)."""
    N, sidx, lidx, G = T
    return np.array([[index(T, g, k) for k in range(N)] for g in range(G)], dtype=np.int64)


def gather(T, full):
    """full [ngroup * G, N] -> x [ngroup, n]; a shared parameter takes data set 0's value."""
    N, sidx, lidx, G = T
    full = np.asarray(full).reshape(-1, G, N)
    x = np.empty((full.shape[0], nouter(T)), dtype=full.dtype)
    for g in range(G - 1, -1, -1):                                      # data set 0 last: its shared values stay
        for k in range(N):
            x[:, index(T, g, k)] = full[:, g, k]
    return x


def expand(T, x):
    """x [n] -> P [G, N];  x [ngroup, n] -> P [ngroup * G, N]."""
    N, sidx, lidx, G = T
    x = np.asarray(x)
    X = x.reshape(-1, nouter(T))
    P = np.empty((X.shape[0], G, N), dtype=X.dtype)
    for g in range(G):
        for k in range(N):
            P[:, g, k] = X[:, index(T, g, k)]
    return P[0] if x.ndim == 1 else P.reshape(-1, N)


def scatter(T, Jf):
    """Inner Jacobians Jf [G] of (m, N) -> J (G m, n): a shared column takes rows g m + i from every data set, the local column
    (g, l) from its own and is +0.0 in every other row."""
    N, sidx, lidx, G = T
    m = Jf[0].shape[0]
    J = np.zeros((G * m, nouter(T)))
    for g in range(G):
        for k in range(N):
            J[g * m:(g + 1) * m, index(T, g, k)] = Jf[g][:, k]
    return J


def stacked(T, residual, jacobian=None):
    """Callbacks (f, j) of oracle.lm_solve for the stacked problem of one group: residual(g, p) -> r [m] and
    jacobian(g, p) -> (m, N) of data set g at its inner parameters p."""
    N, sidx, lidx, G = T

    def f(x, out):
        P = expand(T, x)
        out[:] = np.concatenate([residual(g, P[g]) for g in range(G)])

    def j(x, J):
        P = expand(T, x)
        J[:, :] = scatter(T, [jacobian(g, P[g]) for g in range(G)])
    return f, (j if jacobian is not None else None)
