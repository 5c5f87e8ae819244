"""Parameter maps (include/nonlin_hip.h: nlh_pmap_*) restated in numpy, step by step in the operation order the header
states: one IEEE operation per step, so that the device kernels reproduce every function bit for bit.  A map is the tuple
of tables nlh_pmap_tables reads back -- (kind, index, scale, offset, free_to_full) -- and tables() builds that tuple on its
own from (nfull, fixed, tied), which is what the tests hold the library's read-back to.  Test infrastructure, not part of
the product."""
import numpy as np

FREE, FIXED, TIED = 0, 1, 2


def tables(nfull, fixed=(), tied=None):
    """(kind, index, scale, offset, free_to_full) of a map: free parameters numbered in ascending full index; index[k] the free
    number (free k), the source's full index (tied k) or -1 (fixed k); scale / offset 1.0 / 0.0 where k is not tied."""
    tied = dict(tied or {})
    kind = np.zeros(nfull, dtype=np.int32)
    kind[list(fixed)] = FIXED
    for k in tied:
        kind[k] = TIED
    index = np.full(nfull, -1, dtype=np.int32)
    scale, offset = np.ones(nfull), np.zeros(nfull)
    f2f = np.flatnonzero(kind == FREE).astype(np.int32)
    index[f2f] = np.arange(len(f2f), dtype=np.int32)
    for k, (src, sc, of) in tied.items():
        index[k], scale[k], offset[k] = src, sc, of
    return kind, index, scale, offset, f2f


def expand(T, x, full):
    """free x [n] (or [.., n]) -> full p [N]: free and fixed first, then the ties in ascending k (u = scale p_src; p = u + offset)."""
    kind, index, scale, offset, f2f = T
    x, full = np.asarray(x), np.asarray(full)
    p = np.array(np.broadcast_to(full, x.shape[:-1] + (len(kind),)), dtype=np.result_type(x, full))
    for k in range(len(kind)):
        if kind[k] == FREE:
            p[..., k] = x[..., index[k]]
    for k in range(len(kind)):
        if kind[k] == TIED:
            u = scale[k] * p[..., index[k]]
            p[..., k] = u + offset[k]
    return p


def gather(T, full):
    """full [.., N] -> free x [.., n]."""
    return np.ascontiguousarray(np.asarray(full)[..., T[4]])


def ties_of(T, j):
    """The tied k, ascending, whose source is free unknown j."""
    kind, index, scale, offset, f2f = T
    return [k for k in range(len(kind)) if kind[k] == TIED and index[k] == f2f[j]]


def contract(T, Jf):
    """Inner Jacobian Jf (m, N) -> J (m, n): v = Jf[:, free_to_full[j]]; v = v + scale_k Jf[:, k] over the ties of j, k ascending."""
    kind, index, scale, offset, f2f = T
    cols = []
    for j in range(len(f2f)):
        v = Jf[:, f2f[j]]
        for k in ties_of(T, j):
            v = v + scale[k] * Jf[:, k]
        cols.append(v)
    return np.stack(cols, axis=1)


def factors(T):
    """(j_k, g_k) per full parameter: the free number of k or of its source and the factor; j_k = -1 where there is none."""
    kind, index, scale, offset, f2f = T
    jk, g = np.full(len(kind), -1), np.ones(len(kind))
    for k in range(len(kind)):
        if kind[k] == FREE:
            jk[k] = index[k]
        elif kind[k] == TIED and kind[index[k]] == FREE:
            jk[k], g[k] = index[index[k]], scale[k]
    return jk, g


def cov_expand(T, cov, sigma, failed=False):
    """cov (n, n), sigma (n) of the free unknowns -> (cov_full (N, N), sigma_full (N)): (g_k cov[j_k][j_l]) g_l and
    fabs(g_k) sigma[j_k]; +0.0 where a parameter has no factor; NaN everywhere for a problem that did not solve."""
    jk, g = factors(T)
    N = len(jk)
    if failed:
        return np.full((N, N), np.nan), np.full(N, np.nan)
    cf, sf = np.zeros((N, N)), np.zeros(N)
    for k in range(N):
        if jk[k] < 0:
            continue
        sf[k] = np.fabs(g[k]) * sigma[jk[k]]
        for l in range(N):
            if jk[l] >= 0:
                cf[k, l] = (g[k] * cov[jk[k], jk[l]]) * g[l]
    return cf, sf


def dense(T):
    """The N x n matrix S of the map's linear part: d p / d x."""
    jk, g = factors(T)
    S = np.zeros((len(jk), len(T[4])))
    for k in range(len(jk)):
        if jk[k] >= 0:
            S[k, jk[k]] = g[k]
    return S
